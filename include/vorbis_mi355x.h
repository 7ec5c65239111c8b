/* vorbis_mi355x — C ABI of the MI355X-native batched Vorbis (aoTuV) encode path.
 *
 * Drop-in boundary for the per-block encode path of spvkgn/vorbis-aotuv-lancer
 * (libvorbis 1.3.7 + aoTuV b6.03): vorbis_analysis() -> mapping0_forward() -> {window,
 * mdct_forward, drft_forward, _vp_* psy, floor1_fit/encode, couple/quantise, residue VQ}
 * -> vorbis_bitrate_addblock()/flushpacket().  Plain pointers and sizes only; device
 * pointers are HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Every entry point names the reference interface it replaces (file:line relative to
 * the reference tree).  All functions return 0 on success, a negative VBM_E* otherwise,
 * and never fall back to a CPU path: without a HIP device they fail with VBM_ENODEV.
 *
 * Results are bit-identical to the reference's SCALAR C path (the `#else` branches of
 * `#ifdef __SSE__`), see DESIGN.md.
 */
#ifndef VORBIS_MI355X_H
#define VORBIS_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBM_OK       0
#define VBM_EINVAL  (-131) /* same value as OV_EINVAL, include/vorbis/codec.h:228 */
#define VBM_EFAULT  (-129) /* OV_EFAULT */
#define VBM_EIMPL   (-130) /* OV_EIMPL  */
#define VBM_ENODEV  (-1000)
#define VBM_EHIP    (-1001)

/* library / device ------------------------------------------------------------------ */
const char *vbm_version(void);
/* number of HIP devices visible; <0 on error.  Does not create a context. */
int vbm_device_count(void);
/* last HIP error string seen by this library on the calling thread ("" if none) */
const char *vbm_last_error(void);

/* ---- MDCT ------------------------------------------------------------------------
 * vbm_mdct_plan replaces mdct_lookup (lib/mdct.h:55-73) + mdct_init (lib/mdct.c:54-92):
 * trig tables are computed on the host with libm in double and rounded to float exactly
 * as lib/mdct.c:67-76 does, then kept device-resident.  It also carries the two
 * rising half-windows the block size can meet (lib/window.c:29-2122; b->window[W],
 * lib/block.c:218-219) so that windowing fuses into the transform.
 *
 *   n        transform size: 256, 512, 1024, 2048 or 4096 (the block sizes of the shipped mode families)
 *   short_n  size of the short block of the same mode pair (for n==2048: 256); the
 *            left/right window halves of a long block next to a short one use it
 *   win_n / win_short: host pointers to the rising half-windows (n/2 and short_n/2
 *            floats); may be NULL if only vbm_mdct_forward_batch() will be used.
 */
typedef struct vbm_mdct_plan vbm_mdct_plan;

int vbm_mdct_plan_create(vbm_mdct_plan **plan, int n, int short_n,
                         const float *win_n, const float *win_short);
void vbm_mdct_plan_destroy(vbm_mdct_plan *plan);
/* host copy of the trig table (n + n/4 floats) — for parity tests */
const float *vbm_mdct_plan_trig(const vbm_mdct_plan *plan);

/* Batched mdct_forward(mdct_lookup*, float *in, float *out) — lib/mdct.c:1799 / lib/mdct.h:78.
 *   d_in : nblocks x n   floats, block-major, device
 *   d_out: nblocks x n/2 floats, device
 */
int vbm_mdct_forward_batch(const vbm_mdct_plan *plan, const float *d_in, float *d_out,
                           long nblocks, void *stream);

/* Batched _vorbis_apply_window(pcm, winno, blocksizes, lW, W, nW) + mdct_forward —
 * lib/window.c:2137 + lib/mdct.c:1799 as called from mapping0_forward, lib/mapping0.c:825-843.
 *   d_pcm    : nblocks x n floats (un-windowed block PCM, block-major)
 *   d_wflags : one byte per block, bit0 = lW, bit1 = nW (vb->lW / vb->nW; only read for
 *              long blocks; NULL means every neighbour is long).  Short blocks always
 *              use the full short window (lib/window.c:2139-2140).
 */
int vbm_window_mdct_batch(const vbm_mdct_plan *plan, const float *d_pcm, float *d_out,
                          const uint8_t *d_wflags, long nblocks, void *stream);

/* Batched tonal-estimation transform of mapping0_forward loop A (lib/mapping0.c:825-888):
 * _vorbis_apply_window + drft_forward (lib/smallft.c:6770, FFTPACK scalar path) + the
 * log-power conversion
 *     logfft[0] = scale_dB + todB(re0) + .345 ;  logfft[k] = scale_dB + .5f*todB(re_k^2+im_k^2) + .345
 * and the per-block maximum local_ampmax = min(0, max_k logfft[k]) (:862-888).
 *   d_pcm          : nblocks x n floats (un-windowed)
 *   d_logfft       : nblocks x n/2 floats
 *   d_local_ampmax : nblocks floats
 */
int vbm_window_fft_log_batch(const vbm_mdct_plan *plan, const float *d_pcm, float *d_logfft,
                             float *d_local_ampmax, const uint8_t *d_wflags, long nblocks, void *stream);
/* host copy of the FFTPACK twiddle table (n floats = drft_lookup.trigcache + n) — for parity tests */
const float *vbm_mdct_plan_fft_twiddles(const vbm_mdct_plan *plan);

/* ---- encoder setup ----------------------------------------------------------------------
 * vbm_setup replaces codec_setup_info + the looks of private_state that vorbis_analysis_init()
 * builds (lib/block.c:181-331: _vp_psy_init, floor1_look, res0_look, vorbis_book_init_encode,
 * mdct_init, drft_init).  It is created from two VPK packs shipped with the package:
 *   common_vpk : static tables (windows, ATH, tone masks, dB lookup …)   data/common.vpk
 *   mode_vpk   : the (channels, rate, quality) class, i.e. the output of
 *                vorbis_encode_init_vbr (lib/vorbisenc.c:977)           data/mode_*.vpk
 * Creation is host-only; tables are uploaded when an encoder is created on a device. */
typedef struct vbm_setup_handle vbm_setup_handle;
int vbm_setup_create(vbm_setup_handle **setup, const char *common_vpk, const char *mode_vpk);
void vbm_setup_destroy(vbm_setup_handle *setup);
/* Introspection of the derived look tables by name ("psy/3/ath", "floor/1/sorted_index",
 * "book/7/codelist", "residue/0/partbook", "info", …) for parity checks; *kind is one of
 * 'f' float32, 'i' int32, 'u' uint32, 'b' int8, 'd' float64.  The pointer stays valid until the
 * next call on the same thread (scalars) or until the setup is destroyed (arrays). */
int vbm_setup_table(const vbm_setup_handle *setup, const char *name, const void **data, long *count,
                    char *kind);

/* ---- batched analysis ---------------------------------------------------------------------
 * vbm_encoder holds, on the device, the carried per-stream encoder state of `nstreams` streams
 * (private_state's aoTuV fields mblock/tblock/lownoise_compand_level/lW_block_mode/lW_no/impadnum,
 * lib/codec_internal.h:85-92; vorbis_block_internal.ampmax and vorbis_look_psy_global.ampmax)
 * plus the workspace for batches of up to `max_batch` blocks.
 *
 * vbm_analysis_batch() is the batched form of the reference's per-block sequence
 *     vorbis_analysis(vb, NULL)            lib/analysis.c:29   -> mapping0_forward lib/mapping0.c:738
 *     vorbis_bitrate_addblock(vb)          lib/bitrate.c:73    (VBR: parks the block)
 *     vorbis_bitrate_flushpacket(vd, &op)  lib/bitrate.c:229   (VBR: packetblob[PACKETBLOBS/2])
 * for `nsb` blocks that share one block type, at most one block per stream and call, in the
 * stream's block order (blocks of one stream are order dependent).
 *   block_mode   0 impulse short, 1 padding short, 2 transition long, 3 long
 *                (= blocktype | W<<1, lib/mapping0.c:768-775; vbi->blocktype from lib/block.c:620-638)
 *   stream_ids   host array [nsb]: which stream each block belongs to
 *   wflags       host array [nsb]: bit0 = vb->lW, bit1 = vb->nW
 *   d_pcm        device, [nsb][channels][blocksize] floats: vb->pcm as vorbis_analysis_blockout
 *                hands it over (un-windowed, lib/block.c:653-698)
 *   d_packets    device, [nsb][vbm_encoder_max_packet_bytes()] bytes: op->packet of every block
 *   d_packet_bytes device, [nsb] ints: op->bytes, or -1 if a packet outgrew max_packet_bytes — check it
 *                before using the row (its bytes are then incomplete)
 * A stream id may appear ONCE per call: the blocks of a stream are order dependent and two of them in one
 * batch would race on the carried state; duplicates are rejected with VBM_EINVAL.
 * Managed-bitrate setups (15 packetblobs + reservoirs) go through the same calls: see "Managed bitrate" below. */
typedef struct vbm_encoder vbm_encoder;
int vbm_encoder_create(vbm_encoder **enc, vbm_setup_handle *setup, int nstreams, int max_batch);
void vbm_encoder_destroy(vbm_encoder *enc);
int vbm_encoder_reset(vbm_encoder *enc); /* back to the state after vorbis_analysis_init */
int vbm_encoder_max_packet_bytes(const vbm_encoder *enc);
int vbm_analysis_batch(vbm_encoder *enc, int block_mode, int nsb, const int *stream_ids,
                       const uint8_t *wflags, const float *d_pcm, uint8_t *d_packets,
                       int *d_packet_bytes, void *stream);
/* Two-stream form of vbm_analysis_batch.  The FRONT half of the path (window, MDCT, FFT,
 * psychoacoustics, _vp_offset_and_mix: every kernel that reads or writes the carried per-stream
 * state) is ordered on `stream_front`, the BACK half (floor1_fit/_encode,
 * _vp_couple_quantize_normalize, residue VQ, packet assembly) on `stream_back`; d_pcm must be ready
 * on stream_front, packets are ready on stream_back.  Consecutive calls use alternate workspaces,
 * so with two different streams the back half of one call runs while the front half of the next
 * one does: the back half's few-wavefront kernels (floor fit) and the front half's wide ones
 * share the GPU.  Results are those of vbm_analysis_batch.  stream_back == stream_front is
 * vbm_analysis_batch. */
int vbm_analysis_batch2(vbm_encoder *enc, int block_mode, int nsb, const int *stream_ids,
                        const uint8_t *wflags, const float *d_pcm, uint8_t *d_packets,
                        int *d_packet_bytes, void *stream_front, void *stream_back);

/* One ROUND: blocks of all four block types at once (what one pass of vorbis_analysis_blockout over
 * all streams yields).  counts[m] blocks of type m; stream_ids / wflags (host) grouped by type, type
 * 0 first; d_pcm: the blocks of type m start at float offset (number of blocks of lower types) *
 * channels * blocksizes[1] and lie [count][channels][N_m].  A stream may appear once per round.
 * The four batches run side by side on internal HIP streams (forked from and joined back to
 * `stream`), so the few
 * short blocks of a round cost no more than the long-block batch beside them.  Packets come back in
 * the grouped order: d_packets[k][max_packet_bytes], d_packet_bytes[k]. */
int vbm_analysis_round(vbm_encoder *enc, const int *counts, const int *stream_ids, const uint8_t *wflags,
                       const float *d_pcm, uint8_t *d_packets, int *d_packet_bytes, void *stream);
/* Rounds with a deferred join.  vbm_analysis_round_begin enqueues a round like vbm_analysis_round but does not
 * make `stream` wait for its batches; a later round only waits for those batches of the round before it that
 * its own streams were part of (the blocks of a stream stay in order), so the handful of short blocks of one
 * round runs beside the long-block batch of the previous one.  Outputs are complete on `stream` after
 * vbm_analysis_round_join.  Buffers handed to a round (d_pcm, outputs) may be reused once `stream` has passed
 * vbm_analysis_round_wait_workspace before the round after the next, or a join.  (Reference: the application
 * loop of examples/encoder_example.c:211-235 run for many streams at once; the packets do not depend on how the
 * rounds are scheduled.) */
int vbm_analysis_round_begin(vbm_encoder *enc, const int *counts, const int *stream_ids, const uint8_t *wflags,
                             const float *d_pcm, uint8_t *d_packets, int *d_packet_bytes, void *stream);
int vbm_analysis_round_join(vbm_encoder *enc, void *stream);
/* ... leaving the newest big batch (>= 1024 blocks of one type) pending: only its front half is waited for; its
 * back half (floor, couple/quantise, packets: nothing the next round reads) then runs beside the front half of
 * the next write's big batch.  Its outputs are complete on `stream` after the next lazy join or a full join. */
int vbm_analysis_round_join_lazy(vbm_encoder *enc, void *stream);
int vbm_analysis_round_wait_workspace(vbm_encoder *enc, void *stream);
/* Stage intermediates of the LAST batch as block-major rows ([channel-block][rows]) for parity
 * tests: "mdct_raw" "logfft" "logmdct" "noise" "tone" "logmask" "mdct" "epeak" "npeak" "post"
 * "floor_out" "residue", and the vectors "local_ampmax" "global_ampmax" "post_valid" "nonzero"
 * "poste" "packet_bytes".  d_out may be NULL to query rows/kind ('f' float32, 'i' int32). */
int vbm_encoder_fetch(vbm_encoder *enc, const char *name, void *d_out, long *rows, char *kind, void *stream);

/* Managed bitrate (setups made by vorbis_encode_init: reference lib/vorbisenc.c:997-1070).  With such a
 * setup vbm_analysis_batch / _batch2 / _round and the front end do per block what vorbis_analysis(vb, NULL)
 * + vorbis_bitrate_addblock + vorbis_bitrate_flushpacket do (lib/analysis.c:30-62, lib/bitrate.c:73-252):
 * all PACKETBLOBS (15) packets of the block are produced (lib/mapping0.c:1097-1181, loop :1204), the
 * stream's reservoirs pick one, and that packet — truncated to the ceiling or zero-padded to the floor when
 * max / min rates are set — is the one handed out.  Nothing in the call sequence changes.  For parity tests:
 * packetblob k of the LAST batch as produced, before the choice (d_packets [nsb][max_packet_bytes],
 * d_packet_bytes [nsb]; either may be NULL), and the vector "choice" of vbm_encoder_fetch. */
int vbm_encoder_fetch_blob(vbm_encoder *enc, int k, uint8_t *d_packets, int *d_packet_bytes, void *stream);

/* Sub-batches.  The transforms run on the whole batch; the stages after them run as `n` slices of
 * the batch (multiples of 64 stream-blocks), each on an internal HIP stream forked from and joined
 * back to the caller's stream with events, so that the serial few-wavefront kernels of one slice
 * overlap with the wide kernels of the others.  Results do not depend on n.  Default 1
 * (environment VBM_SUB_BATCHES overrides at create); n = 1 launches everything on the caller's
 * stream.  In the two-stream form (vbm_analysis_batch2 with two different streams) the slices apply to the
 * back half only: the first on stream_back, the others on internal streams joined to it.  Measured on MI355X:
 * every HIP stream beyond four shares a hardware queue with another and costs more than the slices gain, so 1
 * stays the default. */
int vbm_encoder_set_sub_batches(vbm_encoder *enc, int n);
int vbm_encoder_sub_batches(const vbm_encoder *enc);

/* ---- stream front end --------------------------------------------------------
 * What libvorbis does between the application's PCM and vorbis_analysis(), for all `nstreams` of
 * an encoder at once and on the device:
 *   vorbis_analysis_buffer + vorbis_analysis_wrote   (reference include/vorbis/codec.h:192-193,
 *                                                     lib/block.c:405-553: pre_amplitude, LPC
 *                                                     extrapolation of stream start and end)
 *   vorbis_analysis_blockout                          (codec.h:194, lib/block.c:557-812) with the
 *                                                     envelope detector that picks the block sizes
 *                                                     (lib/envelope.c:101-728)
 * followed by vbm_analysis_batch on the blocks that came out.  Usage, mirroring
 * examples/encoder_example.c:190-235:
 *     vbm_frontend_write(fe, d_pcm, vals, q);                       // every stream gets `vals` samples
 *     do vbm_frontend_encode_round(fe, d_pkt, d_len, info, &n, q);  // <= 1 block per stream per round
 *     while (n > 0);
 *     ... vbm_frontend_finish(fe, ids, k, q) = vorbis_analysis_wrote(vd, 0), then rounds until n == 0.
 * Rounds may be deferred (a stream inside a run of short blocks yields up to 8 blocks per 1024
 * samples; blocks and packets do not depend on when the rounds run), but drain completely before
 * vbm_frontend_finish: like the reference (lib/block.c:531-541) it fits the end-of-stream LPC to the
 * samples the buffer holds at that moment.
 * The block sequence (lW, W, nW, block type, granulepos, packetno, e_o_s) and the packets are those
 * of the reference's scalar build for the same PCM.  d_pcm: device float, [nstreams][channels][vals].
 * encode_round: packets of the round in d_packets[k][max_packet_bytes] / d_packet_bytes[k],
 * k < *nblocks, described by info[k] (host array of nstreams entries); blocks are grouped by block
 * type, streams ascending inside a group.  The call synchronises `stream` once (it reads the
 * block decisions back to choose the batches).  Errors: VBM_EINVAL for writes that would overrun
 * the PCM buffer (the reference's OV_EINVAL, lib/block.c:540) or follow finish. */
typedef struct vbm_frontend vbm_frontend;
typedef struct vbm_packet_info {
    int stream;                 /* stream index */
    int block_mode;             /* 0 impulse, 1 padding, 2 transition, 3 long */
    int lW, W, nW;              /* vb->lW, vb->W, vb->nW */
    int eos;                    /* op.e_o_s */
    long long granulepos;       /* op.granulepos */
    long long packetno;         /* op.packetno (audio packets start at 3) */
} vbm_packet_info;
int vbm_frontend_create(vbm_frontend **fe, vbm_encoder *enc);
void vbm_frontend_destroy(vbm_frontend *fe);
int vbm_frontend_reset(vbm_frontend *fe);
int vbm_frontend_write(vbm_frontend *fe, const float *d_pcm, int vals, void *stream);
int vbm_frontend_finish(vbm_frontend *fe, const int *stream_ids, int n, void *stream);
/* Streams that do not move in lock step: write `vals` samples to the listed streams only (d_pcm:
 * [n][channels][vals], one entry per listed stream, a stream at most once per call), and start a
 * new stream in listed slots (state of vorbis_analysis_init for the front end and the encoder;
 * typically after the slot's previous stream has delivered its e_o_s packet). */
int vbm_frontend_write_streams(vbm_frontend *fe, const int *stream_ids, int n, const float *d_pcm, int vals,
                               void *stream);
/* The same with the caller's own layout: channel c of stream_ids[k] at pcm + (by_slot ? stream_ids[k] : k) * stream_stride
 * + c * ch_stride floats (ch_stride >= vals).  pcm may be host memory the device can read (hipHostMalloc): the append
 * kernel fetches it over the bus itself, no staging copy and no separate upload (what the drop-in shim's
 * vorbis_analysis_buffer hands out, reference lib/block.c:405-436).  Returns when the samples have been taken. */
int vbm_frontend_write_streams_strided(vbm_frontend *fe, const int *stream_ids, int n, const float *pcm, int vals,
                                       long stream_stride, long ch_stride, int by_slot, void *stream);
/* A size per stream (whole files in batches: lengths differ, last writes are ragged, slots turn over): channel c of
 * stream_ids[k] is the vals[k] floats at pcm + src_offsets[k] + c * ch_strides[k]; stream_ids, src_offsets, vals and
 * ch_strides are host arrays of n entries, pcm as above (typically one device-resident store of whole files).  It is
 * vorbis_analysis_buffer + vorbis_analysis_wrote(vals[k]) for each listed stream, with the rules of the call above per
 * stream: a stream at most once per call, vals[k] > 0, ch_strides[k] >= vals[k], src_offsets[k] >= 0; VBM_EINVAL after
 * vbm_frontend_finish and if any listed stream's buffer would overrun.  Every check runs before anything is enqueued:
 * a refused call changes no stream.  One upload of n job records and one append launch, whatever the sizes.  Work put
 * on `stream` after the call sees the samples taken (as for vbm_frontend_write); a host that wants to rewrite the
 * source itself synchronises `stream` first. */
int vbm_frontend_write_ragged(vbm_frontend *fe, const int *stream_ids, int n, const float *pcm,
                              const long long *src_offsets, const int *vals, const long long *ch_strides,
                              void *stream);
int vbm_frontend_restart_streams(vbm_frontend *fe, const int *stream_ids, int n, void *stream);
/* Buffer occupancy, for callers that do not drain completely after every write (a stream inside a
 * run of short blocks yields up to 8 blocks per 1024 samples, each in its own round): the most
 * samples any stream holds now, and the occupancy a write may not exceed (VBM_EINVAL beyond it).  The buffer
 * is 24 long blocks per channel (environment VBM_FE_BUFFER_BLOCKS, 8..64, read at create): 3 of them reserved
 * for the end-of-stream padding, a third for the origin of the samples to climb before they are moved back to the
 * start (one copy per several blocks where the reference memmoves after every block), the rest is slack that lets
 * such a stream fall behind and catch up, instead of forcing extra rounds on every write.  (The reference grows its buffer on demand: lib/block.c:424-430.) */
int vbm_frontend_max_buffered(const vbm_frontend *fe);
int vbm_frontend_capacity(const vbm_frontend *fe);
int vbm_frontend_encode_round(vbm_frontend *fe, uint8_t *d_packets, int *d_packet_bytes,
                              vbm_packet_info *info, int *nblocks, void *stream);
/* One round for the listed streams only: every other stream is left alone (no block, no state change), as if
 * its application had not asked vorbis_analysis_blockout yet.  Outputs as vbm_frontend_encode_round. */
int vbm_frontend_encode_round_streams(vbm_frontend *fe, const int *stream_ids, int n, uint8_t *d_packets,
                                      int *d_packet_bytes, vbm_packet_info *info, int *nblocks, void *stream);
/* Packets for a host consumer: the rows d_packets[k][max_packet_bytes] with d_packet_bytes[k] bytes used (k < n)
 * as one byte run in d_out, packet k at d_offsets[k] (4-byte aligned, exclusive prefix sum of the padded
 * lengths), d_offsets[n] = bytes of d_out used; negative lengths count as 0.  d_out needs n * max_packet_bytes
 * bytes in the worst case, d_offsets n + 1 entries.  One D2H copy of d_offsets[n] bytes then replaces n row
 * copies (what vorbis_bitrate_flushpacket's ogg_packet needs on the host, reference lib/bitrate.c:229-252).
 * A packet's run is its length rounded up to 4 bytes; the pad bytes are the row's own.  Nothing of d_out beyond
 * d_offsets[n] is written.  Lengths are at most max_packet_bytes (not checked); max_packet_bytes is a multiple of 4, d_packets
 * and d_out are 4-byte aligned, n >= 0 (VBM_EINVAL otherwise, and for a NULL d_offsets, or with n > 0 any NULL
 * pointer).  n == 0: d_offsets[0] = 0 is written on `stream`, the other pointers are not looked at. */
int vbm_packets_compact(const uint8_t *d_packets, const int *d_packet_bytes, int n, int max_packet_bytes,
                        uint8_t *d_out, long long *d_offsets, void *stream);
/* Up to max_rounds rounds in one call (deferred joins: vbm_analysis_round_begin), results complete on `stream`
 * when the call's work has run: packets / lengths / infos of all rounds, compact, in round order;
 * round_blocks[r] = blocks of round r, *nrounds = rounds that produced blocks.  Rounds stop when one produces
 * nothing, when fewer than `nstreams` of the cap_blocks output slots are left, or — after min_rounds — as
 * soon as every stream could take `headroom` more samples with its buffer at most half full.  Same packets
 * as any other schedule of vbm_frontend_encode_round calls. */
int vbm_frontend_encode_rounds(vbm_frontend *fe, int min_rounds, int max_rounds, int headroom,
                               uint8_t *d_packets, int *d_packet_bytes, vbm_packet_info *info, int cap_blocks,
                               int *round_blocks, int *nrounds, void *stream);
/* The same with a lazy join (vbm_analysis_round_join_lazy): the outputs of the call's big batch are complete on
 * `stream` only after the NEXT vbm_frontend_encode_rounds_lazy call, or vbm_frontend_join; all other outputs as
 * above.  The caller keeps the output buffers of a call untouched until then.  For throughput: the back half of
 * one write's long-block batch overlaps the next write. */
int vbm_frontend_encode_rounds_lazy(vbm_frontend *fe, int min_rounds, int max_rounds, int headroom,
                                    uint8_t *d_packets, int *d_packet_bytes, vbm_packet_info *info, int cap_blocks,
                                    int *round_blocks, int *nrounds, void *stream);
int vbm_frontend_join(vbm_frontend *fe, void *stream);

/* Rounds built on the device: the throughput form of the loop above with NO host in it.  The device decides which
 * streams deliver a block (k_fe_classify), assigns them lanes (k_fe_plan), carves the blocks and runs the per-block
 * path on device-resident counts; the call only enqueues work and returns.  Nothing is read back: the host learns
 * what came out from the outputs, when it chooses to look.
 *   Layout: a round has vbm_device_round_lanes() output slots ("lanes").  Block type m owns a fixed region of
 *   them (the impulse, padding and transition blocks a quarter of the stream count each, then the long blocks with
 *   one lane per stream — half of them in the later rounds of a call, whose long blocks are those of streams catching
 *   up); inside a region the blocks follow in ascending stream order.  A stream whose type's region is
 *   full keeps its block for the next round (rounds may be deferred: blocks and packets do not depend on when they
 *   run); a stream that has fallen behind its input delivers a block in every round of a call until it has caught up.
 *   nrounds rounds per call; round r writes
 *     d_packets      [r][lane][max_packet_bytes]   (may be NULL)
 *     d_packet_bytes [r][lane]   length, -2 = no block in this lane, -1 = packet outgrew the buffer
 *     d_info         [r][lane]   vbm_packet_info of the lane's block (stream = -1: none); device or pinned host memory
 *     d_counts       [r][4]      blocks of each type (device memory: the round's kernels read it while they run)
 *   all complete on `stream` when the call's work has run (lazy = 1: the long-block batch of the call only after
 *   the next call or vbm_frontend_join, as vbm_frontend_encode_rounds_lazy; lazy = 2: nothing is tied to `stream` by
 *   the call — a consumer calls vbm_frontend_join(fe, its_stream) before it reads, so the stream that feeds PCM never
 *   waits for packets).  The buffers belong to the call until then.
 *   With lazy = 2 nothing on the device ties a consumer's reads of a call's buffers to a later call that is given
 *   the same buffers: the caller does.  Either it keeps every read of a buffer set ahead of the call that reuses it,
 *   or it records an event on the consumer's stream behind those reads and makes `stream` wait for that event before
 *   the reusing call (every kernel and copy that writes the four outputs runs on a stream forked from the front end's
 *   own stream after the call has made that stream wait for `stream`, the transforms that run ahead of the state
 *   waits included).  The Python front end's ring of three sets does the second through FrontEnd.release().
 *   The encoder must have been created with max_batch >= vbm_device_round_lanes(setup, nstreams).
 * Mixing with the host-built rounds above is allowed (e.g. to drain completely before vbm_frontend_finish): the first
 * such call waits for the front end's stream and fetches the buffer fills it needs.  While only device-built rounds
 * run, vbm_frontend_write does not check the buffer fill: the caller keeps rounds and writes in balance (two rounds
 * per 1024-sample write keep every stream ahead of its input at the block-switching rates of music; the fill can be
 * watched with vbm_frontend_max_buffered, which synchronises). */
int vbm_device_round_lanes(const vbm_setup_handle *setup, int nstreams);
int vbm_frontend_encode_rounds_device(vbm_frontend *fe, int nrounds, uint8_t *d_packets, int *d_packet_bytes,
                                      vbm_packet_info *d_info, int *d_counts, int lazy, void *stream);
/* The block type every stream had ready when the newest device-built round was planned (-1: none), [nstreams] bytes,
 * copied to `out` (host) on `stream` after the round's outputs: a stream with a type here and no record in the round
 * found its type's lane region full and delivers the block in the next round. */
int vbm_frontend_round_types(vbm_frontend *fe, signed char *out, void *stream);
/* running totals of the device-built rounds: out[0..3] blocks of type 0..3, out[4] samples all streams advanced by,
 * out[5] writes the device refused because a stream's buffer was full (must stay 0: the refused samples are lost —
 * the device-side counterpart of vbm_frontend_write's VBM_EINVAL).  Synchronises the front end's stream. */
int vbm_frontend_device_stats(vbm_frontend *fe, unsigned long long *out);

/* ---- stream wrapper, host only ------------------------------------------------
 * vbm_header_packets = vorbis_analysis_headerout (reference lib/info.c:636-717): the identification,
 * comment and setup header packets of a setup, concatenated in buf with their sizes in lens[3]
 * (buf == NULL: sizes only).  vendor NULL = the string of the reference's scalar build
 * (lib/info.c:43).  They are packets 0..2 of a stream; the audio packets of
 * vbm_frontend_encode_round follow with packetno 3...
 * vbm_ogg_stream_* = libogg's ogg_stream_packetin / ogg_stream_pageout / ogg_stream_flush (libogg is
 * external to the reference; page format per the reference's doc/framing.html): packetin queues a
 * packet with the granulepos / e_o_s of its vbm_packet_info; pageout returns 1 and a pointer to a
 * complete page (valid until the next call) when one is due, 0 otherwise; flush != 0 forces out
 * what is queued (the reference application flushes after the three headers,
 * examples/encoder_example.c:150-157). */
int vbm_header_packets(const vbm_setup_handle *setup, const char *vendor, const char *const *comments,
                       int ncomments, uint8_t *buf, long cap, long *lens);
/* The comment header alone (reference vorbis_commentheader_out, lib/info.c:600-617); buf == NULL: size query. */
int vbm_comment_packet(const char *vendor, const char *const *comments, int ncomments, uint8_t *buf, long cap, long *len);
/* The inverse, host only: .ogg bytes of ONE logical Vorbis stream -> its packets (libogg's ogg_sync_pageout +
 * ogg_stream_pagein + ogg_stream_packetout, as the Python read_ogg).  Pages are checked for the capture pattern, version,
 * CRC, truncation, one serial number, page sequence and the continuation flag: any violation returns VBM_EOGG (message
 * in vbm_last_error) and nothing past data[n) is read.  sizes[5] = the three header packet lengths, the number of audio
 * packets, their total bytes.  Size query with headers == NULL; then call again with sizes as returned and
 *   headers     sizes[0]+sizes[1]+sizes[2] bytes, the header packets back to back
 *   packets     sizes[4] bytes, the audio packets back to back; offsets [sizes[3]+1] (CSR, offsets[0] = 0)
 *   granulepos  [sizes[3]] the page's granule position on the last packet that ends on a page, else -1
 *   eos         [sizes[3]] 1 on the last packet of the end-of-stream page
 * An unterminated packet at the end of the data is dropped.  Fewer than three packets: VBM_EOGG. */
#define VBM_EOGG (-1002)
int vbm_ogg_demux(const uint8_t *data, long n, long *sizes, uint8_t *headers, uint8_t *packets, long long *offsets,
                  long long *granulepos, uint8_t *eos);

/* ---- Ogg demux, batch form: many whole files per call, on the device ----------------------------------------------
 * vbm_ogg_demux for `nfiles` files that lie in one device buffer, file f in d_data[file_offsets[f], file_offsets[f+1])
 * (bytes between files may be left out by the offsets; nothing outside a file's range is read for it).  Every file
 * holds ONE logical stream and is judged by the rules of vbm_ogg_demux, on its own bytes alone: it comes out with status
 * 0 and the header packets, audio packet bytes, offsets, granulepos and eos vbm_ogg_demux gives for it, or with
 * VBM_EOGG exactly when vbm_ogg_demux returns VBM_EOGG, and then adds no packet and no byte.  (One exception that no
 * Vorbis file meets: header packets of 2^31 bytes or more in all are VBM_EOGG, as header_bytes could not hold them.)
 * The protocol is vbm_ogg_demux's size query / fill, per batch:
 *   vbm_ogg_demuxer_create   workspace on the current device for calls of up to max_files files that span up to
 *                            max_bytes bytes (file_offsets[nfiles] - file_offsets[0]): about 1.2 * max_bytes + 120 *
 *                            max_files bytes (csrc/ogg_demux.h).  vbm_host_ogg_demuxer_create: the same in host memory
 *                            for the vbm_host_* calls, touches no device.
 *   vbm_ogg_demux_scan       validates every file, CRCs included: d_info[f].status is final.  d_info[f] also has the
 *                            file's page count, serial number, the three header packet lengths, its audio packets and
 *                            their bytes (all 0 for a failed file), and packet_base / payload_base / header_base, the
 *                            sums of packets / payload_bytes / header bytes over the files in front of it.
 *                            d_totals[3]: audio packets, payload bytes and header bytes of the batch.  d_info and
 *                            d_totals are device memory; file_offsets [nfiles + 1] is host memory and is free on return.
 *   vbm_ogg_demux_fill       writes the outputs of the last scan on this demuxer (d_data must still hold the files).  The
 *                            audio packets of all good files form ONE CSR over a dense payload: packet k of file f is
 *                            d_payload[d_offsets[packet_base + k], d_offsets[packet_base + k + 1]), d_offsets[0] = 0 and
 *                            d_offsets[packet_base + packets] = payload_base + payload_bytes is where the next file
 *                            starts; d_granulepos / d_eos as vbm_ogg_demux, at packet_base + k.  The three header
 *                            packets of file f lie back to back at d_headers + header_base.  This is the input of
 *                            vbm_synthesis_runs with no copy in between: run_packets = packets, d_data = d_payload,
 *                            d_offsets + packet_base of the first file of the call, and so on.
 *                            Capacities: d_headers holds header_cap bytes, d_payload payload_cap bytes, d_offsets
 *                            packet_cap + 1 entries, d_granulepos and d_eos packet_cap.  Nothing is written past any of
 *                            them: when one is below the batch's total, NOTHING is written at all and the demuxer's
 *                            status word becomes VBM_OGG_DEMUX_ECAP (0 after a fill that wrote its outputs).
 *   vbm_ogg_demux_status     the status word of the last fill -> *status (host memory).  The one call here that waits:
 *                            for `stream`, on which that fill must have been enqueued.
 * scan and fill allocate nothing and only enqueue on `stream`; the one wait in scan is for the pinned slot that carried
 * the file offsets two scans earlier.  VBM_EINVAL, with nothing enqueued: nfiles negative or above max_files, a
 * negative or decreasing offset, a span above max_bytes, a null pointer (d_data may be null when the span is 0, d_info
 * when nfiles is 0, an output of fill when its capacity is 0; d_offsets never), a negative capacity, fill without a scan,
 * a host demuxer in a device call or the other way round.
 *   vbm_host_ogg_demux_scan / _fill   the same source on the CPU with host pointers and a host demuxer. */
#define VBM_OGG_DEMUX_ECAP 1
typedef struct {
    int status;                 /* 0 or VBM_EOGG */
    int pages;
    unsigned serialno;
    int header_bytes[3];
    long long packets;          /* audio packets (after the three headers) */
    long long payload_bytes;    /* their bytes */
    long long packet_base, payload_base, header_base;   /* exclusive sums over the files before it */
} vbm_ogg_file_info;
typedef struct vbm_ogg_demuxer vbm_ogg_demuxer;
int vbm_ogg_demuxer_create(vbm_ogg_demuxer **dm, int max_files, long long max_bytes);
int vbm_host_ogg_demuxer_create(vbm_ogg_demuxer **dm, int max_files, long long max_bytes);
void vbm_ogg_demuxer_destroy(vbm_ogg_demuxer *dm);
int vbm_ogg_demux_scan(vbm_ogg_demuxer *dm, int nfiles, const uint8_t *d_data, const long long *file_offsets,
                       vbm_ogg_file_info *d_info, long long *d_totals, void *stream);
int vbm_ogg_demux_fill(vbm_ogg_demuxer *dm, uint8_t *d_headers, long long header_cap, uint8_t *d_payload,
                       long long payload_cap, long long *d_offsets, long long *d_granulepos, uint8_t *d_eos,
                       long long packet_cap, void *stream);
int vbm_ogg_demux_status(vbm_ogg_demuxer *dm, int *status, void *stream);
int vbm_host_ogg_demux_scan(vbm_ogg_demuxer *dm, int nfiles, const uint8_t *data, const long long *file_offsets,
                            vbm_ogg_file_info *info, long long *totals);
int vbm_host_ogg_demux_fill(vbm_ogg_demuxer *dm, uint8_t *headers, long long header_cap, uint8_t *payload,
                            long long payload_cap, long long *offsets, long long *granulepos, uint8_t *eos,
                            long long packet_cap);

/* ---- Ogg chains: where the links of chained files start, for many files per call, on the device ----------------------
 * A chained file is whole logical streams ("links") back to back, and the calls above take one stream per file.  A split
 * finds where the links of `nfiles` files start, file f in d_data[file_offsets[f], file_offsets[f+1]) as above, so that
 * the links can be demuxed as files.  The rule (csrc/ogg_chain.h): link 0 starts at the file's first byte, in every
 * file, an empty one included; then page after page from there, a page that carries the beginning-of-stream flag
 * (header byte 5, bit 0x02) and is not the file's first starts a link.  The walk stops where fewer than 27 bytes are
 * left, the capture pattern is not "OggS", the version is not 0, or the lacing table or the body is not all in front of
 * the file's end, and the rest of the file then belongs to the last link found.  There is no resync.  The split never
 * fails and never judges: CRC, serial number, page sequence and continuation flag stay with the demux of each link,
 * which rejects a link exactly as it would reject those bytes as a file.  A file with no second beginning-of-stream
 * page is one link, the file.  Nothing outside a file's range is read for it.
 *   vbm_ogg_chain_create   workspace on the current device for calls of up to max_files files that span up to max_bytes
 *                          bytes: about 0.3 * max_bytes + 16 * max_files bytes.  vbm_host_ogg_chain_create: the same in
 *                          host memory for vbm_host_ogg_chain_split, touches no device.
 *   vbm_ogg_chain_split    d_file_links [nfiles + 1]: the exclusive sums of the files' link counts, so file f has links
 *                          d_file_links[f] .. d_file_links[f+1] - 1 of the batch and d_file_links[nfiles] = total.
 *                          ALWAYS written.  d_link_offsets, of capacity link_cap + 1 entries: link j of the batch is
 *                          d_data[d_link_offsets[j], d_link_offsets[j+1]), and d_link_offsets[total] =
 *                          file_offsets[nfiles].  When total > link_cap NOTHING is written to d_link_offsets and the
 *                          status word becomes VBM_OGG_DEMUX_ECAP (0 after a split that wrote them).  Both outputs are
 *                          device memory; file_offsets is host memory and is free on return.  d_link_offsets, copied to
 *                          the host, is a valid file_offsets of vbm_ogg_demux_scan with nfiles = total over the same
 *                          d_data.
 *   vbm_ogg_chain_status   the status word of the last split -> *status (host memory); waits for `stream`, on which
 *                          that split must have been enqueued.
 * split allocates nothing and only enqueues on `stream`; its one wait is for the pinned slot that carried the file
 * offsets two splits earlier.  VBM_EINVAL, with nothing enqueued: nfiles negative or above max_files, a negative or
 * decreasing offset, a span above max_bytes, a null pointer (d_data may be null when the span is 0), a negative
 * link_cap, a host object in a device call or the other way round.
 *   vbm_host_ogg_chain_split   the same source on the CPU with host pointers and a host object. */
typedef struct vbm_ogg_chain vbm_ogg_chain;
int vbm_ogg_chain_create(vbm_ogg_chain **ch, int max_files, long long max_bytes);
int vbm_host_ogg_chain_create(vbm_ogg_chain **ch, int max_files, long long max_bytes);
void vbm_ogg_chain_destroy(vbm_ogg_chain *ch);
int vbm_ogg_chain_split(vbm_ogg_chain *ch, int nfiles, const uint8_t *d_data, const long long *file_offsets,
                        long long *d_file_links, long long *d_link_offsets, long long link_cap, void *stream);
int vbm_ogg_chain_status(vbm_ogg_chain *ch, int *status, void *stream);
int vbm_host_ogg_chain_split(vbm_ogg_chain *ch, int nfiles, const uint8_t *data, const long long *file_offsets,
                             long long *file_links, long long *link_offsets, long long link_cap);

/* ---- Tolerant Ogg demux: many whole files that may be damaged, chained or both, on the device ------------------------
 * Every call above is strict: one violated page rule gives the file or link VBM_EOGG.  A resync demux delivers what
 * rules 1 to 4 and 6 of the resync feed ("Resync mode" below) deliver from each file pushed whole with `end`; rule 5 (stops)
 * and the slot capacities do not exist here.  Per file, from its first byte: the walk goes to the next "OggS" (a version
 * byte other than 0 moves it on one byte); a candidate whose 27 header bytes, lacing table or body do not all lie in
 * the file ends the file there; a whole candidate with a bad CRC moves the walk on one byte, one with a good CRC by its
 * size, so a capture pattern inside a good page is never looked at.  Rules 2 to 4 (whose page, discontinuity, link
 * start) apply to the good pages unchanged.  The ENTRIES of the batch are the links whose three header packets
 * completed, in order: file f has entries d_file_links[f] .. d_file_links[f+1] - 1, possibly none, and an entry's status
 * is always 0.  A gap mark (1) is on the first audio packet of every link but the file's first and on the first packet
 * completed behind every discontinuity.
 *   vbm_ogg_resync_create   workspace on the current device for calls of up to max_files files that span up to
 *                           max_bytes bytes and hold up to max_candidates capture patterns: about 248 * max_candidates
 *                           + max_bytes / 1024 + 56 * max_files bytes (csrc/ogg_resync.h).  Patterns cannot overlap, so
 *                           max_bytes / 4 always suffices; real files have about one per 4 KB.
 *                           vbm_host_ogg_resync_create: the same in host memory, touches no device.
 *   vbm_ogg_resync_scan     d_events [nfiles]: per file, beginning-of-stream pages taken, those whose link is no entry,
 *                           gap marks set, bytes skipped, good pages ignored, pages taken.  d_file_links [nfiles + 1].
 *                           d_info, of capacity entry_cap: per entry a vbm_ogg_file_info as vbm_ogg_demux_scan gives it.
 *                           d_totals [6]: entries, audio packets, payload bytes, header bytes, candidates found, and
 *                           the scan's status: 0, or VBM_OGG_DEMUX_ECAP when the candidates exceed max_candidates (then
 *                           only d_totals[4] and [5] are written) or the entries exceed entry_cap (then d_info is not
 *                           written; everything else is).  The counts are exact: a second try with them succeeds.  All
 *                           four are device memory; file_offsets is host memory and is free on return.
 *   vbm_ogg_resync_fill     as vbm_ogg_demux_fill over the entries, with one more output d_gap [packet_cap].  After a
 *                           scan that ended in VBM_OGG_DEMUX_ECAP, or with a capacity below the batch's total, NOTHING
 *                           is written and the status word becomes VBM_OGG_DEMUX_ECAP.
 *   vbm_ogg_resync_status   the status word of the last scan or fill -> *status (host memory); waits for `stream`.
 * scan and fill allocate nothing and only enqueue on `stream`; VBM_EINVAL, with nothing enqueued, as for
 * vbm_ogg_demux_scan / _fill, and for a negative entry_cap or max_candidates.  A crafted file of nested false headers
 * makes the CRC work quadratic in its size, as it does for the reference's sequential page seek.
 *   vbm_host_ogg_resync_scan / _fill   the same source on the CPU with host pointers and a host object. */
typedef struct {
    int links_started, links_bad;
    long long gaps, skipped_bytes, ignored_pages, pages;
} vbm_ogg_resync_events;
typedef struct vbm_ogg_resync vbm_ogg_resync;
int vbm_ogg_resync_create(vbm_ogg_resync **rs, int max_files, long long max_bytes, long long max_candidates);
int vbm_host_ogg_resync_create(vbm_ogg_resync **rs, int max_files, long long max_bytes, long long max_candidates);
void vbm_ogg_resync_destroy(vbm_ogg_resync *rs);
int vbm_ogg_resync_scan(vbm_ogg_resync *rs, int nfiles, const uint8_t *d_data, const long long *file_offsets,
                        vbm_ogg_resync_events *d_events, long long *d_file_links, vbm_ogg_file_info *d_info,
                        long long entry_cap, long long *d_totals, void *stream);
int vbm_ogg_resync_fill(vbm_ogg_resync *rs, uint8_t *d_headers, long long header_cap, uint8_t *d_payload,
                        long long payload_cap, long long *d_offsets, long long *d_granulepos, uint8_t *d_eos,
                        uint8_t *d_gap, long long packet_cap, void *stream);
int vbm_ogg_resync_status(vbm_ogg_resync *rs, int *status, void *stream);
int vbm_host_ogg_resync_scan(vbm_ogg_resync *rs, int nfiles, const uint8_t *data, const long long *file_offsets,
                             vbm_ogg_resync_events *events, long long *file_links, vbm_ogg_file_info *info,
                             long long entry_cap, long long *totals);
int vbm_host_ogg_resync_fill(vbm_ogg_resync *rs, uint8_t *headers, long long header_cap, uint8_t *payload,
                             long long payload_cap, long long *offsets, long long *granulepos, uint8_t *eos, uint8_t *gap,
                             long long packet_cap);

/* ---- Ogg stream selection: the Vorbis stream of multiplexed files, for many files per call, on the device -------------
 * A multiplexed file carries the pages of several logical streams interleaved (.ogv: Theora beside Vorbis; Skeleton,
 * Kate or CMML tracks beside the audio), and the calls above take one stream per file.  A selection copies, for each of
 * `nfiles` files, file f in d_data[file_offsets[f], file_offsets[f+1]) as above, the pages of its Vorbis stream to
 * d_out and drops the rest, so that what comes out is a plain Vorbis file, or a plain chained one for
 * vbm_ogg_chain_split.  Pages are copied whole: CRCs, page numbers and granule positions stay as they are.  The rule
 * (csrc/ogg_select.h), page after page with the parse test and the stops of the chain split: a page is a head page if it
 * carries the beginning-of-stream flag or is the file's first; a head page behind a page that is none starts a new group
 * (a chain boundary), in which nothing is chosen yet; the first head page of a group whose body begins with the 7 bytes
 * 01 "vorbis" chooses its serial number for the group; a page is kept if and only if a stream is chosen and the page
 * carries its serial number.  At a stop the rest of the file is kept if a stream is chosen there.  So the first Vorbis
 * stream of a group wins (as in the reference's vorbisfile.c), a group without one keeps nothing, and a plain Vorbis
 * file or chain comes out byte for byte as it went in.  The selection never fails and never judges: CRC, page sequence,
 * continuation flags and header packets stay with the demux.  There is no resync, and nothing outside a file's range is
 * read for it.
 *   vbm_ogg_select_create   workspace on the current device for calls of up to max_files files that span up to max_bytes
 *                           bytes: about 0.9 * max_bytes + 24 * max_files bytes.  vbm_host_ogg_select_create: the same
 *                           in host memory for vbm_host_ogg_select, touches no device.
 *   vbm_ogg_select          d_out_offsets [nfiles + 1]: the exclusive sums of the files' kept bytes from 0 on, so the
 *                           output of file f is d_out[d_out_offsets[f], d_out_offsets[f+1]) and d_out_offsets[nfiles] =
 *                           total; with d_out as d_data it is a valid file_offsets of vbm_ogg_chain_split and
 *                           vbm_ogg_demux_scan.  d_info [nfiles]: one record per file.  Both are ALWAYS written.  d_out,
 *                           of capacity out_cap bytes: the size of the input, file_offsets[nfiles] - file_offsets[0],
 *                           always suffices.  It must not overlap the files: the selection is not done in place.  When
 *                           total > out_cap NOTHING is written to d_out and the status word becomes
 *                           VBM_OGG_DEMUX_ECAP (0 after a selection that wrote it).  The outputs are device memory;
 *                           file_offsets is host memory and is free on return.
 *   vbm_ogg_select_status   the status word of the last selection -> *status (host memory); waits for `stream`, on
 *                           which that selection must have been enqueued.
 * select allocates nothing, reads nothing back and only enqueues on `stream`; its one wait is for the pinned slot that
 * carried the file offsets two calls earlier.  VBM_EINVAL, with nothing enqueued: nfiles negative or above max_files, a
 * negative or decreasing offset, a span above max_bytes, a null pointer (d_data may be null when the span is 0, d_out
 * when out_cap is 0, d_info when nfiles is 0), a negative out_cap, an output that overlaps the files, a host object in
 * a device call or the other way round.
 *   vbm_host_ogg_select     the same source on the CPU with host pointers and a host object.
 * VBM_OGG_SELECT_CHUNK: the bytes of d_out that one block of the copy kernel writes (its grid is sized from the input). */
#define VBM_OGG_SELECT_CHUNK 16384
typedef struct {
    long long kept_bytes;       /* bytes of the file that are kept: pages, and the tail behind a stop */
    long long kept_pages;       /* pages kept */
    long long foreign_pages;    /* pages dropped */
    int streams;                /* groups in which a Vorbis stream was chosen; 0: the file has none and keeps nothing */
    int foreign_streams;        /* head pages that were dropped */
    uint32_t first_serial;      /* serial number of the first chosen stream (0 without one) */
    int reserved;               /* 0 */
} vbm_ogg_select_info;
typedef struct vbm_ogg_selector vbm_ogg_selector;
int vbm_ogg_select_create(vbm_ogg_selector **sel, int max_files, long long max_bytes);
int vbm_host_ogg_select_create(vbm_ogg_selector **sel, int max_files, long long max_bytes);
void vbm_ogg_select_destroy(vbm_ogg_selector *sel);
int vbm_ogg_select(vbm_ogg_selector *sel, int nfiles, const uint8_t *d_data, const long long *file_offsets, uint8_t *d_out,
                   long long out_cap, long long *d_out_offsets, vbm_ogg_select_info *d_info, void *stream);
int vbm_ogg_select_status(vbm_ogg_selector *sel, int *status, void *stream);
int vbm_host_ogg_select(vbm_ogg_selector *sel, int nfiles, const uint8_t *data, const long long *file_offsets, uint8_t *out,
                        long long out_cap, long long *out_offsets, vbm_ogg_select_info *info);

/* ---- Ogg demux, incremental form: the next bytes of many live streams per call, on the device -----------------------
 * A feed holds max_streams stream slots.  Every call takes, for each slot of a list, a chunk of bytes of any length (0
 * included) cut anywhere, and returns the audio packets those bytes completed, as ONE CSR grouped by stream in list
 * order: the input of vbm_synthesis_runs with no copy in between.  The three header packets of a stream are kept in its
 * slot for vbm_ogg_feed_headers.  The rules are those of vbm_ogg_demux, applied as the bytes arrive:
 *   - a stream's run is what it carried over from earlier calls followed by the call's chunk; pages are taken from it in
 *     order.  A page header is judged once its 27 bytes are present (capture pattern, version 0, one serial number, page
 *     sequence from 0, continuation flag against an open packet), the CRC once the page is whole.
 *   - a page that is not yet whole is no error: its bytes are carried.  A packet that is open at the end of the last
 *     whole page is carried too and comes out, carried bytes first, in the call that completes it.
 *   - granulepos / eos as vbm_ogg_demux: the last packet that ends on a page gets the page's, the others -1 and 0.
 *   - a violation: packets completed on the pages in front of the offending page, in the same call included, are
 *     delivered, nothing of that page is; the slot's status becomes VBM_EOGG and stays so until the slot is reset.
 *     Bytes for a slot with a status, or after its `end`, are ignored.
 *   - end[i] != 0 says no more bytes will come: VBM_EOGG if a partial page is left or fewer than three packets were
 *     completed; a packet still open is dropped.
 *   - three capacities per slot, fixed at create: max_page_carry, the bytes of an incomplete trailing page (1..65307);
 *     max_packet_bytes, the bytes of an open audio packet at the end of a page; header_cap, the three header packets
 *     together (an open header packet included).  A page that would exceed the second or third is not taken, a tail
 *     above the first is not carried, and the slot gets the sticky status VBM_OGG_FEED_EBIG.  The two stores are judged
 *     page by page, so their outcome does not depend on where the calls cut the stream.  Other slots are not touched.
 *   - slots that a call does not list keep their state.  vbm_ogg_feed_reset_streams frees slots for new streams.
 * The protocol is size query, then fill, per call:
 *   vbm_ogg_feed_create      state and workspace on the current device: per slot 72 + max_page_carry + max_packet_bytes
 *                            + header_cap bytes; per feed about 2.2 * max_call_bytes + (max_page_carry + 260) *
 *                            max_streams (csrc/ogg_feed.h).  vbm_host_ogg_feed_create: the same in host memory for the
 *                            vbm_host_* calls, touches no device.
 *   vbm_ogg_feed_scan        ids [n] (host): the slots, each at most once; chunk i is d_data[chunk_offsets[i],
 *                            chunk_offsets[i+1]) (device bytes, host offsets [n + 1]); end [n] (host) or NULL for all 0.
 *                            Writes d_info[i] (device) for list entry i: the slot's status after the call, headers_ready
 *                            and header_bytes (0 until ready), serialno, the audio packets / payload bytes this call
 *                            completes and their exclusive sums over the list, pending (bytes of the incomplete page it
 *                            carries on) and consumed (bytes of the whole pages taken, carried bytes included).
 *                            d_totals[2] (device): packets and payload bytes of the call.  The chunks are copied: d_data is
 *                            free once the scan has run.  It changes no stream state.
 *   vbm_ogg_feed_fill        writes the CSR of the last scan: d_payload, d_offsets [packets + 1] (d_offsets[0] = 0, entry
 *                            i's packets from packet_base on), d_granulepos, d_eos; then commits every listed slot's new
 *                            carry and state.  d_payload holds payload_cap bytes, d_offsets packet_cap + 1 entries,
 *                            d_granulepos and d_eos packet_cap.  When one is below the call's total NOTHING is written,
 *                            the status word becomes VBM_OGG_DEMUX_ECAP and every slot stays as it was: the same scan
 *                            can be filled again with larger buffers.  A fill that wrote leaves 0; a further fill of a
 *                            scan that is already committed writes nothing and leaves VBM_EINVAL in the status word.
 *   vbm_ogg_feed_status      the status word of the last fill -> *status (host).  Waits for `stream`.
 *   vbm_ogg_feed_headers     sizes[3] and, unless headers is NULL, the three header packets of a slot back to back
 *                            (cap bytes of host memory).  Waits for `stream`.  VBM_EINVAL while the slot has not completed
 *                            three packets, or when cap is too small.
 *   vbm_ogg_feed_reset_streams   ids [n] (host): those slots are fresh again (any serial number, sequence from 0).
 * scan and fill allocate nothing and only enqueue on `stream`; the one wait in scan (and reset) is for the pinned slot
 * that carried the arguments two calls earlier.  VBM_EINVAL, with nothing enqueued: n negative or above max_streams, an
 * id out of range or listed twice, a negative or decreasing offset, more than max_call_bytes bytes, a null pointer
 * (d_data may be null when there are no bytes, d_info when n is 0, d_payload / d_granulepos / d_eos when their capacity
 * is 0), a negative capacity, fill without a scan, a host feed in a device call or the other way round.
 *   vbm_host_ogg_feed_scan / _fill   the same source on the CPU with host pointers and a host feed; _status, _headers,
 *                            _reset_streams and _destroy take both kinds.
 *
 * Resync mode (vbm_ogg_feed_create2 with VBM_OGG_FEED_RESYNC; flags = 0 is vbm_ogg_feed_create) is the tolerant form for a
 * live mount: it follows a chain of logical streams (links), joins a stream mid-way and goes on after lost or damaged
 * pages, as libogg's ogg_sync_pageseek / ogg_stream_pagein do.  scan and fill are used as before; the rules differ
 * (stated once in csrc/ogg_feed.h, oggfeed_rs_walk):
 *   1 finding a page: at the walk's position a page header is "OggS" and version 0.  Without one the walk moves to the
 *     next "OggS" of the run and counts the bytes passed as skipped; with none in the run its last 3 bytes are carried
 *     (they may begin one).  A candidate whose header, lacing table or body is not all present is carried, within
 *     max_page_carry (above it: VBM_OGG_FEED_EBIG, as in strict mode; only 65307 is immune to a false header that claims
 *     a long page).  A whole candidate has its CRC checked at once; with a bad CRC the walk resumes one byte on and the
 *     candidate counts as skipped bytes.
 *   2 whose page: a page with a good CRC and the beginning-of-stream flag is a link start.  Any other page is ignored
 *     (and counted) when its serial number is not the current link's, when no link is open, when the link is bad (see 3)
 *     or has delivered its end-of-stream page.
 *   3 a page of the link whose sequence number is not the expected one, or whose continuation flag does not match
 *     whether a packet is open, is a discontinuity page: the open packet is dropped; if the flag says continued, the
 *     leading segments through the first lacing value below 255 belong to no packet; the expected sequence becomes the
 *     page's plus 1; the next packet completed carries a gap mark.  While the link's headers are open (fewer than three
 *     packets) the link becomes bad instead: nothing more of it is delivered, headers_ready stays 0 and the slot waits
 *     for the next link start.  That is no status.
 *   4 a link start closes the current link, drops an open packet, zeroes the counts and takes the page's serial and
 *     sequence number.  The header store is refilled: headers_ready is 0 until the new link's third packet completes,
 *     then vbm_ogg_feed_headers returns the new link's headers.  The first audio packet of every link after the slot's
 *     first carries a gap mark: the caller switches or restarts its decoder there.
 *   5 a link start or a discontinuity page is taken only as the first page a call takes for the slot.  Met later it ends
 *     the slot's walk in front of it: unvisited bytes of the carried tail stay the tail, unvisited bytes of the chunk are
 *     reported as `left`, and the caller pushes chunk[len - left:] again (that push takes the stopping page first).  So
 *     one call delivers, per slot, packets of one link with nothing lost between them: at most the first carries a mark.
 *     A call takes at most chunk / 27 + 1 pages for a slot (its page records): the carried tail can hold whole pages,
 *     behind a candidate that claimed more bytes than it had, and the page after the last record ends the walk the same
 *     way.
 *   6 `end` is honoured only when left == 0 and the walk did not end at a stop: a partial page or an open packet is
 *     dropped and the slot is done.  After a stop with `end` given, push again (with no bytes if left == 0) while
 *     pending > 0.  The only statuses are VBM_OGG_FEED_EBIG and VBM_EINVAL; VBM_EOGG does not occur.
 *   vbm_ogg_feed_create2     vbm_ogg_feed_create with flags: 0, or VBM_OGG_FEED_RESYNC (16 bytes more per slot); any other
 *                            bit is VBM_EINVAL.
 *   vbm_ogg_feed_scan_events  between scan and fill: d_events[i] (device) for list entry i of the last scan.  VBM_EINVAL
 *                            without a scan, and on a strict feed.
 *   vbm_ogg_feed_fill_gaps   vbm_ogg_feed_fill plus d_gap [packet_cap] (uint8, device; NULL: no marks are written):
 *                            1 when something was lost between the slot's previous delivered packet and this one.
 *                            vbm_ogg_feed_fill on a resync feed drops the marks; on a strict feed fill_gaps writes zeros.
 *   vbm_host_ogg_feed_create2 / _scan_events / _fill_gaps   the host twin.
 *
 * Multiplexed mode (vbm_ogg_feed_create2 with VBM_OGG_FEED_MULTIPLEXED, alone or together with VBM_OGG_FEED_RESYNC) is for
 * mounts that carry other logical streams beside the audio: Theora video, an Ogg Skeleton track, Kate or CMML text.  It
 * applies the rule of vbm_ogg_select (above) as the bytes arrive, per slot, in front of the feed's own rules (stated once
 * in csrc/ogg_feed.h): of every group of streams the first whose first packet is a Vorbis identification header is the
 * slot's stream, and every page of another stream is foreign.  A foreign page is stepped over whole, once it is whole:
 * nothing of it reaches a packet, a store or a status.  Until then it is carried like any page, so max_page_carry has to
 * cover the largest foreign page too (above it: VBM_OGG_FEED_EBIG).  8 bytes more per slot; vbm_ogg_feed_reset_streams
 * makes a slot fresh, with a new group and nothing chosen.  Every call, struct and status is as without the flag.
 *   - strict: the feed does what a strict feed does on the bytes vbm_ogg_select keeps.  Foreign pages are not
 *     CRC-checked.  A chain is still VBM_EOGG, at the second group's Vorbis head page and not before; that page, like
 *     every head page that has to show the Vorbis mark, is judged once it is whole.  Bytes that are no page header (27
 *     are present; capture pattern, version) are VBM_EOGG whether or not a stream has been chosen: unlike a file, a feed
 *     has no end at which to drop them.  `end` with no Vorbis stream is VBM_EOGG (fewer than three packets).
 *   - resync: rule 1 is unchanged, and only pages with a good CRC are told apart.  Rule 2 becomes: a link start is a
 *     page with the beginning-of-stream flag that the rule above keeps.  A foreign page, beginning-of-stream or not,
 *     is ignored and counted in ignored_pages; it closes no link, drops no open packet and sets no gap mark.  A mount
 *     joined mid-way ignores what comes before the next group, whose Vorbis head page starts link 0.
 * The value is 4: tests pin flags 2 and 3 as VBM_EINVAL, so bit 1 stays invalid, and so is every bit from 8 up. */
#define VBM_OGG_FEED_EBIG (-1003)
#define VBM_OGG_FEED_RESYNC 1u
#define VBM_OGG_FEED_MULTIPLEXED 4u
typedef struct {
    int status;                 /* 0, VBM_EOGG or VBM_OGG_FEED_EBIG */
    int headers_ready;
    int header_bytes[3];
    unsigned serialno;
    long long packets;          /* audio packets this call completes */
    long long payload_bytes;    /* their bytes */
    long long packet_base, payload_base;   /* exclusive sums over the list entries before it */
    long long pending;          /* bytes of the incomplete trailing page */
    long long consumed;         /* bytes of the whole pages this call takes */
} vbm_ogg_feed_info;
typedef struct {                /* resync mode: what a scan met for one list entry */
    int link;                   /* the link the call's packets belong to, from 0 over the slot's life (0 too before the first starts) */
    int link_started;           /* the first page this call took began a link */
    int link_bad;               /* the link lost a page while its headers were open */
    int gaps;                   /* packets of this call that carry a gap mark */
    long long skipped_bytes;    /* bytes the call passed that belong to no page with a good CRC */
    long long ignored_pages;    /* pages with a good CRC that were ignored */
    long long left;             /* bytes at the end of the chunk that the call did not look at */
} vbm_ogg_feed_events;
typedef struct vbm_ogg_feed vbm_ogg_feed;
int vbm_ogg_feed_create(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                        int max_packet_bytes, int header_cap);
int vbm_host_ogg_feed_create(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                             int max_packet_bytes, int header_cap);
void vbm_ogg_feed_destroy(vbm_ogg_feed *fd);
int vbm_ogg_feed_scan(vbm_ogg_feed *fd, int n, const int *ids, const uint8_t *d_data, const long long *chunk_offsets,
                      const uint8_t *end, vbm_ogg_feed_info *d_info, long long *d_totals, void *stream);
int vbm_ogg_feed_fill(vbm_ogg_feed *fd, uint8_t *d_payload, long long payload_cap, long long *d_offsets,
                      long long *d_granulepos, uint8_t *d_eos, long long packet_cap, void *stream);
int vbm_ogg_feed_status(vbm_ogg_feed *fd, int *status, void *stream);
int vbm_ogg_feed_headers(vbm_ogg_feed *fd, int id, uint8_t *headers, long long cap, int *sizes, void *stream);
int vbm_ogg_feed_reset_streams(vbm_ogg_feed *fd, int n, const int *ids, void *stream);
int vbm_host_ogg_feed_scan(vbm_ogg_feed *fd, int n, const int *ids, const uint8_t *data, const long long *chunk_offsets,
                           const uint8_t *end, vbm_ogg_feed_info *info, long long *totals);
int vbm_host_ogg_feed_fill(vbm_ogg_feed *fd, uint8_t *payload, long long payload_cap, long long *offsets,
                           long long *granulepos, uint8_t *eos, long long packet_cap);

int vbm_ogg_feed_create2(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                         int max_packet_bytes, int header_cap, unsigned flags);
int vbm_host_ogg_feed_create2(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                              int max_packet_bytes, int header_cap, unsigned flags);
int vbm_ogg_feed_scan_events(vbm_ogg_feed *fd, vbm_ogg_feed_events *d_events, void *stream);
int vbm_host_ogg_feed_scan_events(vbm_ogg_feed *fd, vbm_ogg_feed_events *events);
int vbm_ogg_feed_fill_gaps(vbm_ogg_feed *fd, uint8_t *d_payload, long long payload_cap, long long *d_offsets,
                           long long *d_granulepos, uint8_t *d_eos, uint8_t *d_gap, long long packet_cap, void *stream);
int vbm_host_ogg_feed_fill_gaps(vbm_ogg_feed *fd, uint8_t *payload, long long payload_cap, long long *offsets,
                                long long *granulepos, uint8_t *eos, uint8_t *gap, long long packet_cap);

typedef struct vbm_ogg_stream vbm_ogg_stream;
int vbm_ogg_stream_create(vbm_ogg_stream **os, int serialno);
void vbm_ogg_stream_destroy(vbm_ogg_stream *os);
int vbm_ogg_stream_packetin(vbm_ogg_stream *os, const uint8_t *packet, long bytes, int e_o_s, long long granulepos);
int vbm_ogg_stream_pageout(vbm_ogg_stream *os, int flush, const uint8_t **page, long *bytes);

/* ---- stream wrapper, device form: paging for every stream of an encoder at once ---------------------------------
 * The same pages as vbm_ogg_stream_* makes, byte for byte, for `nstreams` streams per call and without a host in the
 * loop: the call consumes what vbm_frontend_encode_rounds_device (or _encode_round / _encode_rounds) leaves in device
 * memory and leaves one compact byte run per stream, ready to append to that stream's file or socket.  One D2H copy
 * per write then carries finished Ogg pages.  Rule, state sizes and the output bound: csrc/ogg_mux.h.
 *   vbm_ogg_mux_create       state for `nstreams` streams on the current device.  max_packet_bytes: the largest packet a
 *                            row may carry (vbm_encoder_max_packet_bytes).  max_rows_per_stream: the most rows one
 *                            stream may have in one call (0 = 16, at most 64; a device-built call yields at most its
 *                            `nrounds`).  queue_bytes: body bytes a stream may keep queued between calls, 0 = the most
 *                            the paging rule can leave, min(254 * 255, max(4 * max_packet_bytes, 4096 + max_packet_bytes)).
 *   vbm_host_ogg_mux_create  the same with the state in host memory, for vbm_host_ogg_mux_packets: touches no device.
 *   vbm_ogg_mux_start_streams  host code: a new stream starts in each listed slot (at most once per call) with its serial
 *                            number.  Returns the header pages of the listed streams (the three header packets of the
 *                            setup, then a flush: examples/encoder_example.c:139-157) back to back in host_buf, those
 *                            of stream_ids[k] at host_offsets[k] .. host_offsets[k+1]; host_buf == NULL only fills
 *                            host_offsets [n+1] (size query) and resets nothing.  Otherwise the slots' state becomes
 *                            "header pages written, queue empty" (device mux: on `stream`, complete on return).
 *   vbm_ogg_mux_packets      rows k < nrows: packet at d_packets + k * packet_stride, d_packet_bytes[k] bytes (negative: no
 *                            packet), d_info[k] (stream < 0: none), in no stream order; inside a stream the order is
 *                            info.packetno.  flush != 0 acts as ogg_stream_flush for every stream after its packets.
 *                            Outputs: the pages of stream s at d_out + d_offsets[s] .. d_offsets[s+1], d_offsets[nstreams]
 *                            = bytes written; d_status[s] = VBM_MUX_* of stream s, d_status[nstreams] = rows whose
 *                            stream index was >= nstreams (ignored).  out_capacity must be at least
 *                            vbm_ogg_mux_out_bound(mux, nrows), the most a call with nrows rows can emit (VBM_EINVAL
 *                            otherwise, before anything is enqueued).  The call synchronises nothing, allocates
 *                            nothing and runs on `stream`.
 *   vbm_host_ogg_mux_packets the same on the CPU with host pointers and a host mux (no device needed).
 * A stream with a status other than VBM_MUX_OK takes no packet from the failing one on: VBM_MUX_ESTATE for a row of a
 * stream that has not been started or is past its e_o_s (vbm_ogg_stream_packetin's VBM_EINVAL; the state is unchanged);
 * VBM_MUX_EROWS (more rows than max_rows_per_stream: none is taken), VBM_MUX_EQUEUE (queue_bytes exceeded) and
 * VBM_MUX_EPACKET (a packet above max_packet_bytes) lose data and stay set until the slot is started again.  Other
 * streams are not affected. */
#define VBM_MUX_OK      0
#define VBM_MUX_EROWS   1
#define VBM_MUX_EQUEUE  2
#define VBM_MUX_ESTATE  3
#define VBM_MUX_EPACKET 4
typedef struct vbm_ogg_mux vbm_ogg_mux;
int vbm_ogg_mux_create(vbm_ogg_mux **mux, const vbm_setup_handle *setup, int nstreams, int max_packet_bytes,
                       int max_rows_per_stream, int queue_bytes);
int vbm_host_ogg_mux_create(vbm_ogg_mux **mux, const vbm_setup_handle *setup, int nstreams, int max_packet_bytes,
                            int max_rows_per_stream, int queue_bytes);
void vbm_ogg_mux_destroy(vbm_ogg_mux *mux);
int vbm_ogg_mux_start_streams(vbm_ogg_mux *mux, const int *stream_ids, int n, const int *serialnos, const char *vendor,
                              const char *const *comments, int ncomments, uint8_t *host_buf, long long cap,
                              long long *host_offsets, void *stream);
long long vbm_ogg_mux_out_bound(const vbm_ogg_mux *mux, int nrows);
int vbm_ogg_mux_packets(vbm_ogg_mux *mux, const uint8_t *d_packets, long long packet_stride, const int *d_packet_bytes,
                        const vbm_packet_info *d_info, int nrows, int flush, uint8_t *d_out, long long out_capacity,
                        long long *d_offsets, int *d_status, void *stream);
int vbm_host_ogg_mux_packets(vbm_ogg_mux *mux, const uint8_t *packets, long long packet_stride, const int *packet_bytes,
                             const vbm_packet_info *info, int nrows, int flush, uint8_t *out, long long out_capacity,
                             long long *offsets, int *status);

/* Per-stage timing of vbm_analysis_batch: HIP events are recorded between the pipeline's kernels,
 * on the stream each kernel is launched on, for the next `max_calls` calls; profile_end waits for
 * the device and returns the summed milliseconds per stage over all launches
 * (vbm_encoder_stage_count() entries, names from vbm_encoder_stage_name) and the number of calls
 * covered.  The first three stages are launched once per call, the others once per sub-batch. */
int vbm_encoder_profile_begin(vbm_encoder *enc, int max_calls);
int vbm_encoder_profile_end(vbm_encoder *enc, float *stage_ms, int *ncalls);
/* stream-blocks covered by the stage times gathered since vbm_encoder_profile_begin (for a round — vbm_analysis_round*,
 * the front end — the stages of its largest batch are the ones timed); read before vbm_encoder_profile_end */
long long vbm_encoder_profile_blocks(const vbm_encoder *enc);
int vbm_encoder_stage_count(void);
const char *vbm_encoder_stage_name(int k);

/* Host-only table builders (no device needed): the lookup tables the plans upload, for
 * integrators and for CPU-side parity checks.
 *   vbm_host_mdct_trig     n + n/4 floats  (mdct_init, lib/mdct.c:67-76)
 *   vbm_host_fft_twiddles  n floats        (drfti1,   lib/smallft.c:5576-5644; = trigcache + n) */
int vbm_host_mdct_trig(int n, float *out);
/*   vbm_host_book_lattice  {quantvals, minval, delta} of a maptype-1 codebook header, as vorbis_book_init_encode
 *                          derives them (lib/sharedbook.c:303-317: _book_maptype1_quantvals, _float32_unpack) */
int vbm_host_book_lattice(long q_min, long q_delta, long entries, int dim, int *out);
int vbm_host_fft_twiddles(int n, float *out);

/* Bench helper: time `iters` back-to-back launches of vbm_window_mdct_batch with HIP
 * events recorded on `stream` (the stream the kernel runs on).  *ms_total receives the
 * elapsed milliseconds for all iters. */
int vbm_window_mdct_time(const vbm_mdct_plan *plan, const float *d_pcm, float *d_out,
                         const uint8_t *d_wflags, long nblocks, int iters, void *stream,
                         float *ms_total);

/* ---- decode: Vorbis packets -> PCM for many streams -------------------------------------------------------
 * The decode half of the reference, batched like the encode path.  One call takes one audio packet for each of up to
 * max_batch streams that share one set of headers and returns, per row, the PCM that became final with that packet:
 * vorbis_synthesis + vorbis_synthesis_blockin + vorbis_synthesis_pcmout + vorbis_synthesis_read
 * (reference lib/synthesis.c:25-91, lib/block.c:897-1190; examples/decoder_example.c).
 * Not supported (VBM_EIMPL at setup): floor type 0, block sizes outside 256..4096, more than 8 channels.  No chained
 * streams; seeking is by sample windows of a range store (vbm_synthesis_ranges); a live stream gets them through a
 * live range store, which keeps its last packets (vbm_live_store_*, "live range store" below).  Half-rate
 * decoding (vorbis_synthesis_halfrate) is a property of the decoder: vbm_decoder_create_halfrate below.  The
 * reference's own vorbis_synthesis* names are not exported. */
#define VBM_ENOTVORBIS (-132) /* OV_ENOTVORBIS, include/vorbis/codec.h:229-233 */
#define VBM_EBADHEADER (-133) /* OV_EBADHEADER */
#define VBM_EVERSION   (-134) /* OV_EVERSION   */
#define VBM_ENOTAUDIO  (-135) /* OV_ENOTAUDIO  */
#define VBM_EBADPACKET (-136) /* OV_EBADPACKET */

typedef struct vbm_decode_setup vbm_decode_setup;
typedef struct vbm_decoder vbm_decoder;

/* Host only, no device needed: the three header packets, back to back in `headers` with lengths lens[3] ->
 * decode setup (vorbis_synthesis_headerin x3, lib/info.c:237-498, and vorbis_book_init_decode).  Returns 0,
 * VBM_ENOTVORBIS, VBM_EBADHEADER, VBM_EVERSION or VBM_EIMPL. */
int  vbm_decode_setup_create(vbm_decode_setup **ds, const uint8_t *headers, const long *lens);
void vbm_decode_setup_destroy(vbm_decode_setup *ds);
int  vbm_decode_setup_info(const vbm_decode_setup *ds, int *channels, long *rate, int *blocksizes /*[2]*/, int *modes);
/* counts[4] = books, floors, residues, mappings of the setup header */
int  vbm_decode_setup_counts(const vbm_decode_setup *ds, int *counts);
/* Host instance of the device's packet unpack (the same source, csrc/decode.h), for parity tests.  Returns the row
 * status (0, VBM_ENOTAUDIO, VBM_EBADPACKET).  Outputs, all optional except info:
 *   info[4]       mode, W, lW, nW
 *   floor_index   [channels][blocksizes[1]/2] floor line as indices into FLOOR1_fromdB_LOOKUP; 0 on channels whose
 *                 floor is not coded and beyond blocksizes[W]/2
 *   residue       [channels][blocksizes[1]/2] decoded residue before inverse coupling, 0 beyond blocksizes[W]/2
 *   floor_used    [channels] nonzero flag after its propagation over the coupling pairs (mapping0_inverse) */
int  vbm_host_unpack_packet(const vbm_decode_setup *ds, const uint8_t *packet, long bytes, int *info,
                            int *floor_index, float *residue, int *floor_used);

/* Device.  nstreams streams of state (previous block size, overlap tail [channels][blocksizes[1]/2], granulepos, sample
 * count) live on the device.  Without a HIP device: VBM_ENODEV. */
int  vbm_decoder_create(vbm_decoder **dec, const vbm_decode_setup *ds, int nstreams, int max_batch);
/* Half-rate decoding (the reference's vorbis_synthesis_halfrate, lib/synthesis.c:166-179, and
 * ov_halfrate): halfrate 1 makes a decoder whose PCM comes out at rate / 2.  Packets are unpacked at their full block
 * size; the inverse MDCT of a block has half its size and reads the lower half of its spectrum, the windows are those
 * of the halved sizes, and every length below that is blocksizes[1]/2 for a full-rate decoder is blocksizes[1]/4:
 *   vbm_synthesis_batch      d_pcm [nsb][channels][blocksizes[1]/4]; a packet of block size W after one of lW
 *                            returns (blocksizes[lW]/4 + blocksizes[W]/4) / 2 samples
 *   vbm_synthesis_runs       pcm_stride >= max(run_packets) * blocksizes[1]/4
 *   vbm_range_store_create   indexes the streams at the decoder's rate; totals, and the starts / lengths / got of
 *                            vbm_synthesis_ranges, are output samples of the half-rate linear decode (and so do
 *                            vbm_range_store_create_device and vbm_decode_index_device)
 * Granule positions stay in full-rate samples, as in the reference: a packet whose granulepos asks for `extra`
 * full-rate samples less loses extra / 2 (rounded down) output samples (lib/block.c:1112-1118, 1140-1150).  The
 * invariants stated below hold unchanged: any split of a stream into runs and single-packet calls gives the same
 * bits, and a range is bit for bit the slice of the linear decode.  vbm_decoder_fetch returns the full-rate
 * intermediates ("spectrum" is computed on all blocksizes[W]/2 bins; the transform reads the first blocksizes[W]/4).
 * halfrate 0 is vbm_decoder_create; any other value is VBM_EINVAL (checked before the device is looked for).  Every
 * setup the decoder accepts can be decoded at half rate (the reference refuses block sizes <= 64).
 * vbm_decoder_halfrate: the flag the decoder was created with. */
int  vbm_decoder_create_halfrate(vbm_decoder **dec, const vbm_decode_setup *ds, int nstreams, int max_batch,
                                 int halfrate);
int  vbm_decoder_halfrate(const vbm_decoder *dec);
/* Mixed decoders: streams of different header classes in one call.  The decoder is made from caps, not
 * from a setup: up to max_classes classes (vbm_decoder_add_class) of up to max_channels channels (1..8) and blocks of up
 * to max_blocksize (a power of two in 256..4096); halfrate as in vbm_decoder_create_halfrate.  Every stream is bound to
 * a class (vbm_decoder_bind_streams) before its first packet, and may be bound to another at any time.
 * vbm_synthesis_batch, vbm_synthesis_runs and vbm_synthesis_runs_gaps then take streams of any mix of classes in one
 * call, and each stream's d_samples, d_status, d_run_samples and PCM are bit for bit those of a decoder of its class
 * alone.  The rows are those of the caps: d_pcm is [nsb][max_channels][max_blocksize/2] (/4 at half rate) for
 * vbm_synthesis_batch and [nruns][max_channels][pcm_stride] for runs, of which a stream writes its class's channels and
 * samples and nothing else; pcm_stride >= max over the runs of run_packets[r] * blocksizes[1]/2 (/4) of run r's class.
 * A call that lists a stream not bound to a class is VBM_EINVAL and enqueues nothing.  vbm_decoder_reset,
 * vbm_decoder_restart_streams and vbm_decoder_halfrate work as on any decoder (a reset keeps classes and bindings).
 * Not built for mixed decoders, VBM_EINVAL with a message: vbm_synthesis_ranges, vbm_range_store_create,
 * vbm_range_store_create_device, vbm_decode_index_device, vbm_decoder_fetch.
 * vbm_decoder_add_class: copies the setup to the device, enqueued on `stream`, and returns its slot of the class table
 *   in *class_id (0, 1, ...).  Slots are never rewritten or removed, so calls in flight stay valid; calls that use the
 *   class must follow on `stream` or after it.  VBM_EINVAL: the class is over a cap, or the table is full.
 * vbm_decoder_bind_streams: stream stream_ids[i] (distinct, n <= max_batch) is of class class_ids[i] from here on, and
 *   restarts as by vbm_decoder_restart_streams: enqueued on `stream`, in order with the calls before and after it. */
int  vbm_decoder_create_mixed(vbm_decoder **dec, int max_classes, int max_channels, int max_blocksize, int nstreams,
                              int max_batch, int halfrate);
int  vbm_decoder_add_class(vbm_decoder *dec, const vbm_decode_setup *ds, int *class_id, void *stream);
int  vbm_decoder_bind_streams(vbm_decoder *dec, int n, const int *stream_ids /*host*/, const int *class_ids /*host*/,
                              void *stream);
void vbm_decoder_destroy(vbm_decoder *dec);
/* every stream back to its initial state (device idle afterwards) */
int  vbm_decoder_reset(vbm_decoder *dec);
/* vorbis_synthesis_restart (lib/block.c:814) for n streams, enqueued on `stream` */
int  vbm_decoder_restart_streams(vbm_decoder *dec, int n, const int *stream_ids /*host*/, void *stream);
/* One packet for each of nsb streams (ids distinct: duplicates are VBM_EINVAL), enqueued on `stream` (no host
 * synchronisation).  Row k: d_packets + k*packet_stride, d_packet_bytes[k] bytes, granulepos d_granulepos[k] (NULL:
 * all -1), end of stream d_eos[k] (NULL: none).  Outputs: d_pcm [nsb][channels][blocksizes[1]/2] floats, d_samples[k]
 * samples per channel, d_status[k] = 0, VBM_ENOTAUDIO or VBM_EBADPACKET.  A row with an error returns 0 samples and
 * leaves its stream untouched; the first packet of a stream (or after a restart) returns 0 samples; with granulepos /
 * eos the output is trimmed as lib/block.c:1084-1161 trims it. */
int  vbm_synthesis_batch(vbm_decoder *dec, int nsb, const int *stream_ids /*host*/,
                         const uint8_t *d_packets, long packet_stride, const int *d_packet_bytes,
                         const long long *d_granulepos, const uint8_t *d_eos,
                         float *d_pcm, int *d_samples, int *d_status, void *stream);
/* Many packets per stream per call: run r is run_packets[r] (>= 0) consecutive packets of stream stream_ids[r] (ids
 * distinct), in stream order.  Rows are the runs concatenated, P = sum(run_packets) <= max_batch.  Packets are CSR:
 * packet k is d_data[d_offsets[k] .. d_offsets[k+1]), clamped to [0, data_bytes) (nothing outside is read);
 * d_granulepos / d_eos [P] as above.  Outputs: d_pcm [nruns][channels][pcm_stride], run r's PCM contiguous from sample
 * 0, d_run_samples[r] samples per channel; per packet, d_samples[k] and d_status[k] exactly as vbm_synthesis_batch
 * reports them.  For any split of a stream's packets into runs and vbm_synthesis_batch calls, the concatenated PCM,
 * samples and status are bit-for-bit those of one packet per call: the per-stream state (tail, previous block size,
 * granulepos, sample count) is shared, and vbm_decoder_restart_streams applies between calls of either kind.
 * Enqueued on `stream`; no host synchronisation (the run table goes through a pinned staging slot, as the ids of
 * vbm_synthesis_batch).  VBM_EINVAL: a stream id twice or out of range, P > max_batch, a negative count,
 * pcm_stride < max(run_packets) * blocksizes[1]/2. */
int  vbm_synthesis_runs(vbm_decoder *dec, int nruns, const int *stream_ids /*host, distinct*/,
                        const int *run_packets /*host, >= 0*/,
                        const uint8_t *d_data, const long long *d_offsets /*[P+1]*/, long long data_bytes,
                        const long long *d_granulepos /*[P] or NULL*/, const uint8_t *d_eos /*[P] or NULL*/,
                        float *d_pcm, long pcm_stride, int *d_run_samples /*[nruns]*/,
                        int *d_samples /*[P]*/, int *d_status /*[P]*/, void *stream);
/* vbm_synthesis_runs with a gap mark per packet (vbm_ogg_feed_fill_gaps writes them): d_gap[k] != 0 says packets were
 * lost in front of packet k, and before it is laid in the stream's granule position and sample count become -1, as
 * vorbis_synthesis_blockin does at v->sequence + 1 != vb->sequence (lib/block.c:911-915).  The overlap tail and the
 * previous block size are kept, as the reference keeps them.  A mark on a row with an error goes to the stream's next
 * valid packet, in this call or a later one: that packet follows a lost one too.  d_gap NULL is vbm_synthesis_runs. */
int  vbm_synthesis_runs_gaps(vbm_decoder *dec, int nruns, const int *stream_ids /*host, distinct*/,
                             const int *run_packets /*host, >= 0*/,
                             const uint8_t *d_data, const long long *d_offsets /*[P+1]*/, long long data_bytes,
                             const long long *d_granulepos /*[P] or NULL*/, const uint8_t *d_eos /*[P] or NULL*/,
                             const uint8_t *d_gap /*[P] or NULL*/,
                             float *d_pcm, long pcm_stride, int *d_run_samples /*[nruns]*/,
                             int *d_samples /*[P]*/, int *d_status /*[P]*/, void *stream);
/* ---- seekable range decoding ----
 * A stream's linear decode is the PCM of all its packets decoded in order from a fresh stream, one packet per call
 * (what vbm_synthesis_runs returns for the whole stream); output position t is its sample t.
 *
 * Host only, no device needed: the index of one stream's npackets demuxed packets (CSR as for vbm_synthesis_runs,
 * clamped to [0, data_bytes); granulepos / eos NULL: all -1 / 0), from a fresh stream state.  Per packet: status[k]
 * (0, VBM_ENOTAUDIO, VBM_EBADPACKET: the header bits decide it, as in the device unpack), samples[k] (what the linear
 * decode returns for it) and out_start[k] (the exclusive prefix sum of samples); *total = the stream's length
 * (ov_pcm_total).  Reads only each packet's header bits, its granulepos and its eos flag. */
int  vbm_decode_index(const vbm_decode_setup *ds, long long npackets, const uint8_t *data, const long long *offsets,
                      long long data_bytes, const long long *granulepos, const uint8_t *eos, int *status,
                      int *samples, long long *out_start, long long *total);
/* The index of a decoder created with the same `halfrate` (0 or 1, otherwise VBM_EINVAL): samples, out_start and
 * *total in its output samples.  With halfrate 0 this is vbm_decode_index. */
int  vbm_decode_index_halfrate(const vbm_decode_setup *ds, int halfrate, long long npackets, const uint8_t *data,
                               const long long *offsets, long long data_bytes, const long long *granulepos,
                               const uint8_t *eos, int *status, int *samples, long long *out_start, long long *total);
/* A range store: the packets of nstreams streams decoded by `dec` (one set of headers), kept in device memory with
 * their index.  Host inputs, the demuxed streams back to back: stream i is packets stream_packets[i] ..
 * stream_packets[i+1] (stream_packets[0] = 0, non-decreasing), packet k is data[offsets[k] .. offsets[k+1]) clamped to
 * [0, data_bytes), granulepos / eos [stream_packets[nstreams]] or NULL.  The store belongs to `dec`; destroy it
 * before the decoder.  vbm_range_store_totals: totals[nstreams], each stream's linear decode length. */
typedef struct vbm_range_store vbm_range_store;
int  vbm_range_store_create(vbm_range_store **st, vbm_decoder *dec, int nstreams, const long long *stream_packets,
                            const uint8_t *data, const long long *offsets, long long data_bytes,
                            const long long *granulepos, const uint8_t *eos);
void vbm_range_store_destroy(vbm_range_store *st);
int  vbm_range_store_totals(const vbm_range_store *st, long long *totals);
/* The same from a CSR that is already in device memory (what vbm_ogg_demux_fill writes): no packet byte crosses to the
 * host.  The index is built by gfx950 kernels, one lane per packet for the header bits and one wavefront per stream
 * for the running sample counts (64 packets per step; a stream with a granulepos below -1 on a valid packet is walked
 * by one lane instead), bit for bit what vbm_decode_index_halfrate gives for each stream alone.
 *
 * vbm_decode_index_device: the index alone, at the decoder's halfrate, into the caller's device arrays: d_status,
 * d_begin, d_end [P] (a valid packet's part [begin, end) of its block is what the linear decode returns for it:
 * samples = end - begin; 0, 0 for a failed packet), d_out_start [P], d_totals [nstreams].  stream_packets is a host
 * array, read before the call returns.  Only enqueues on `stream`: no allocation, and no wait but for a staging slot
 * that is still in flight from four uploads back (the streams' first packets go up through the decoder's staging
 * ring, at most 4 * max_batch or 2 * nstreams of the decoder per launch).  d_begin is also the kernels' workspace: it holds W between the two.  VBM_EINVAL, with nothing enqueued,
 * on the conditions of vbm_range_store_create, or a NULL output.
 *
 * vbm_host_decode_index_scan: the CPU twin on host arrays (no device needed): the same 64-packet steps, the lanes as
 * a loop.
 *
 * vbm_range_store_create_device: the store of vbm_range_store_create.  It owns copies of the bytes and offsets, made
 * device to device on `stream`; status, out_start + samples and the totals are read back in one copy (12 B per
 * packet) for the host planner of vbm_synthesis_ranges, and that is the call's one wait: when it returns, the
 * caller's arrays are free. */
int  vbm_decode_index_device(vbm_decoder *dec, int nstreams, const long long *stream_packets /*host [nstreams+1]*/,
                             const uint8_t *d_data, const long long *d_offsets /*[P+1]*/, long long data_bytes,
                             const long long *d_granulepos /*[P] or NULL*/, const uint8_t *d_eos /*[P] or NULL*/,
                             int *d_status, int *d_begin, int *d_end, long long *d_out_start, long long *d_totals,
                             void *stream);
int  vbm_host_decode_index_scan(const vbm_decode_setup *ds, int halfrate, int nstreams,
                                const long long *stream_packets, const uint8_t *data, const long long *offsets,
                                long long data_bytes, const long long *granulepos, const uint8_t *eos, int *status,
                                int *begin, int *end, long long *out_start, long long *totals);
int  vbm_range_store_create_device(vbm_range_store **st, vbm_decoder *dec, int nstreams,
                                   const long long *stream_packets /*host*/, const uint8_t *d_data,
                                   const long long *d_offsets, long long data_bytes, const long long *d_granulepos,
                                   const uint8_t *d_eos, void *stream);
/* The same four for a mixed decoder (vbm_decoder_create_mixed): stream_classes [nstreams] (host) is the class of each
 * stream, an id vbm_decoder_add_class has returned for this decoder; any other id is VBM_EINVAL with a message, before
 * anything is allocated or enqueued.  A store's classes are its own: they are not taken from vbm_decoder_bind_streams,
 * and a class added after one store was made may be used by the next.  The index of every stream is the one its
 * class's setup gives for it alone, bit for bit.  The index kernels are the same two launches whatever the number of
 * classes: a packet finds its stream, hence its class, by a search in the staged table of first packets, and a
 * wavefront takes its stream's block sizes from the class table (per launch at most 2 * max_batch or nstreams of the
 * decoder streams).  vbm_host_decode_index_scan_mixed: the CPU twin over setups[nclasses], with the same lookup;
 * VBM_EINVAL for a class id outside [0, nclasses).  stream_classes NULL: the call without _mixed.
 * The plain four refuse a mixed decoder, and these refuse a decoder of one setup (VBM_EINVAL). */
int  vbm_range_store_create_mixed(vbm_range_store **st, vbm_decoder *dec, int nstreams, const long long *stream_packets,
                                  const int *stream_classes /*host [nstreams]*/, const uint8_t *data,
                                  const long long *offsets, long long data_bytes, const long long *granulepos,
                                  const uint8_t *eos);
int  vbm_range_store_create_device_mixed(vbm_range_store **st, vbm_decoder *dec, int nstreams,
                                         const long long *stream_packets /*host*/,
                                         const int *stream_classes /*host [nstreams]*/, const uint8_t *d_data,
                                         const long long *d_offsets, long long data_bytes,
                                         const long long *d_granulepos, const uint8_t *d_eos, void *stream);
int  vbm_decode_index_device_mixed(vbm_decoder *dec, int nstreams, const long long *stream_packets /*host [nstreams+1]*/,
                                   const int *stream_classes /*host [nstreams]*/, const uint8_t *d_data,
                                   const long long *d_offsets /*[P+1]*/, long long data_bytes,
                                   const long long *d_granulepos /*[P] or NULL*/, const uint8_t *d_eos /*[P] or NULL*/,
                                   int *d_status, int *d_begin, int *d_end, long long *d_out_start, long long *d_totals,
                                   void *stream);
int  vbm_host_decode_index_scan_mixed(int nclasses, const vbm_decode_setup *const *setups, int halfrate, int nstreams,
                                      const long long *stream_packets, const int *stream_classes, const uint8_t *data,
                                      const long long *offsets, long long data_bytes, const long long *granulepos,
                                      const uint8_t *eos, int *status, int *begin, int *end, long long *out_start,
                                      long long *totals);
/* Sample windows of the store's streams.  Range r is stream stream_ids[r], start starts[r] >= 0, length lengths[r]
 * >= 0 (host arrays; ranges may repeat and overlap).  got[r] (host) = clamp(total - start, 0, length), and
 *   d_pcm[r][c][0 .. got[r]) == linear decode of the stream [c][start .. start + got[r])   bit for bit;
 * nothing else of d_pcm [nranges][channels][pcm_stride] is written.  Reads and writes no stream state of the decoder:
 * range calls and vbm_synthesis_batch / _runs calls may be interleaved.  Each range decodes the packets that cover it
 * plus one pre-roll packet; a range of more than max_batch packets is cut into pieces, and pieces are packed into
 * sub-calls of at most max_batch rows, all enqueued on `stream` (the piece table of each goes through the staging
 * ring).  VBM_EINVAL, with nothing enqueued: a store of another decoder, a stream id out of range, a negative start
 * or length, pcm_stride < max(lengths), max_batch < 2.
 * A mixed decoder takes the stores its _mixed creators made for it: d_pcm is [nranges][max_channels][pcm_stride], the
 * layout of vbm_synthesis_runs on such a decoder, and range r writes channels 0 .. channels(class of its stream) - 1,
 * samples 0 .. got[r] - 1 and nothing else.  The sub-calls are the same whatever the number of classes, one launch
 * chain each; no stream state is read or written, and the bindings of vbm_decoder_bind_streams play no part. */
int  vbm_synthesis_ranges(vbm_decoder *dec, const vbm_range_store *st, int nranges, const int *stream_ids,
                          const long long *starts, const int *lengths, float *d_pcm, long pcm_stride, int *got,
                          void *stream);
/* Intermediates of the LAST call, per row, padded to blocksizes[1]/2 per channel (as vbm_encoder_fetch):
 *   "info" int [nsb][4]; "floor_index" int, "residue" float, "spectrum" float [nsb][channels][blocksizes[1]/2]
 *   (spectrum: after inverse coupling and the floor multiply, before the IMDCT); "floor_used" int [nsb][channels].
 * d_out NULL: only *rows (values per channel row, 4 for "info") and *kind ('i' / 'f') are returned. */
int  vbm_decoder_fetch(vbm_decoder *dec, const char *name, void *d_out, long *rows, char *kind, void *stream);

/* ---- Ogg cut: sample windows of a range store's streams as new Ogg Vorbis files, no packet decoded or re-encoded -------
 * Range r is stream stream_ids[r] of the store, start starts[r] >= 0, length lengths[r] >= 0 in the store's output
 * samples (host arrays; ranges may repeat and overlap).  Output r is a whole Ogg Vorbis file whose decode is the window:
 * the range's header pages as given, then the store's packets pre .. m unchanged (the packets vbm_synthesis_ranges would
 * decode for the window, pre-roll included), paged and given granule positions so that a Vorbis decoder drops the samples
 * in front of the start and stops at the end (csrc/ogg_cut.h has the rule; reference lib/block.c:1084-1157 is what the
 * decoder does with it).  Both ends are exact, except for a window inside ONE packet: its start moves back to that
 * packet's first sample.  got_starts[r], got_lengths[r] (host): the window the file holds, got_lengths[r] =
 * clamp(total - start, 0, length) (+ the move); 0 gives an empty output, status 0.
 *   vbm_ogg_cut_create      workspace on the current device for calls of up to max_ranges ranges, max_out_bytes output
 *                           bytes and max_header_bytes of header page sets: about 0.17 * max_out_bytes + 250 * max_ranges +
 *                           3 * max_header_bytes bytes (two thirds of the last pinned host memory).
 *                           vbm_host_ogg_cut_create: the same in host memory for vbm_host_ogg_cut_ranges, no device.
 *   vbm_ogg_cut_ranges      header_pages[header_offsets[e], header_offsets[e + 1]), e < nheaders (host,
 *                           header_offsets[0] = 0): sets of whole Ogg pages as the host writer makes them of a stream's
 *                           three header packets (vbm_ogg_stream_*: the identification packet alone on the first page,
 *                           a flush behind the third packet), under any serial number.  Output r opens with set
 *                           header_ids[r] (NULL: r), so the cuts of one source file share one set; serialnos[r] (NULL:
 *                           r) is written into its pages and each page's CRC corrected, which gives the pages the
 *                           writer makes under that serial number.  The audio pages carry the same serial number and
 *                           page numbers that run on from the header pages.  A set that no non-empty output uses is
 *                           only checked for whole pages.
 *                           d_out_offsets [nranges + 1]: exclusive sums of the output sizes, output r is
 *                           d_out[d_out_offsets[r], d_out_offsets[r + 1]).  d_status [nranges + 1]: per range 0 or
 *                           VBM_OGG_CUT_ESHAPE (refused: the output is empty, and its length counts as 0 whatever
 *                           got_lengths[r] says: the refusal is found on the device); d_status[nranges] is the call's
 *                           status word.  Both are ALWAYS written.  When the total exceeds out_cap (0 is allowed, and
 *                           asks for the sizes) NOTHING is written to d_out and the status word is VBM_OGG_CUT_ECAP.
 *                           Refused: packets pre .. k that do not fit one page, a packet behind k (or k itself when the
 *                           window lies inside it) whose start the source trimmed, offsets that are no CSR inside the
 *                           store's data (csrc/ogg_cut.h (a) - (d)).  A store with e_o_s in front of a stream's last
 *                           packet is not covered.
 * cut_ranges allocates no device or pinned memory, reads nothing back and only enqueues on `stream`; its one wait is for the pinned slot that
 * carried the arguments two calls earlier.  VBM_EINVAL, with nothing enqueued: a stream id out of range, a negative
 * start or length, nranges negative or above max_ranges, out_cap negative or above max_out_bytes, header pages above
 * max_header_bytes or not whole pages, decreasing header_offsets, a header id out of range, a null pointer, an output that overlaps the store's
 * data, a half-rate store (its positions are not packet granule positions), a host object in a device call or the other
 * way round.
 *   vbm_host_ogg_cut_ranges the same source on the CPU.  The index comes as plain host arrays (first [nstreams + 1]; status,
 *                           begin, out_end [P]; totals [nstreams]; data, offsets [P + 1]): neither a device nor a packet
 *                           that decodes is needed.  It knows the refusals and writes got_lengths[r] = 0 for them. */
#define VBM_OGG_CUT_ECAP   VBM_OGG_DEMUX_ECAP
#define VBM_OGG_CUT_ESHAPE 2
typedef struct vbm_ogg_cutter vbm_ogg_cutter;
int  vbm_ogg_cut_create(vbm_ogg_cutter **cut, int max_ranges, long long max_out_bytes, long long max_header_bytes);
int  vbm_host_ogg_cut_create(vbm_ogg_cutter **cut, int max_ranges, long long max_out_bytes, long long max_header_bytes);
void vbm_ogg_cut_destroy(vbm_ogg_cutter *cut);
int  vbm_ogg_cut_ranges(vbm_ogg_cutter *cut, const vbm_range_store *st, int nranges, const int *stream_ids,
                        const long long *starts, const long long *lengths, const int *serialnos, int nheaders,
                        const uint8_t *header_pages, const long long *header_offsets, const int *header_ids,
                        uint8_t *d_out, long long out_cap,
                        long long *d_out_offsets, int *d_status, long long *got_starts, long long *got_lengths,
                        void *stream);
int  vbm_host_ogg_cut_ranges(vbm_ogg_cutter *cut, int nstreams, const long long *first, const int *status, const int *begin,
                             const long long *out_end, const long long *totals, const uint8_t *data,
                             const long long *offsets, long long data_bytes, int nranges, const int *stream_ids,
                             const long long *starts, const long long *lengths, const int *serialnos, int nheaders,
                             const uint8_t *header_pages, const long long *header_offsets, const int *header_ids,
                             uint8_t *out, long long out_cap,
                             long long *out_offsets, int *out_status, long long *got_starts, long long *got_lengths);

/* ---- live range store: an appendable range store for live feeds (csrc/live_store.h) ------------------------------------
 * A vbm_range_store with a fixed region per stream: max_packets packet slots and max_bytes payload bytes in device
 * memory.  It takes appended runs of packets, in the arguments of vbm_synthesis_runs_gaps, and drops the oldest packets
 * when a region is full.  vbm_synthesis_ranges, vbm_ogg_cut_ranges, vbm_range_store_totals and vbm_range_store_destroy
 * take it as they take any store.
 *   Positions are output samples since the slot's last restart, at the decoder's rate: the concatenation of what
 *   vbm_synthesis_runs_gaps returns for the same packets, granule positions, e_o_s flags and gap marks in the same order.
 *   totals[i] is its end; first_sample[i] is out_end of the first retained valid packet, which serves only as pre-roll
 *   (no valid packet retained: totals[i]; a fresh slot: 0).  A window that starts at or behind first_sample[i] is bit for
 *   bit the slice of the linear decode; one that starts in front of it gets got = 0 (a cut: an empty output, length 0).
 *   vbm_live_store_create   for a decoder of one setup; _create_mixed for one of vbm_decoder_create_mixed, whose slots
 *                           have no class until vbm_live_store_restart gives them one.  Memory: about nstreams *
 *                           (max_bytes + 32 * max_packets) bytes.  max_bytes < 2^31 - 64, nstreams * (max_packets + 1)
 *                           < 2^31 - 1.
 *   vbm_live_store_append   entry e: run_packets[e] >= 0 consecutive packets for slot stream_ids[e] (host arrays, ids
 *                           distinct, n <= nstreams), the entries' packets concatenated in one CSR on the device (d_data,
 *                           d_offsets [P + 1], d_granulepos / d_eos / d_gap [P] or NULL).  The index goes on from the
 *                           slot's carried state, so how a stream is split over appends does not show.  Per entry
 *                           (host, any may be NULL): status[e] 0, VBM_LIVE_EBIG (a run of more than max_packets packets or
 *                           max_bytes bytes: the slot is left as it was, the other entries are appended) or VBM_EINVAL
 *                           (its offsets are no CSR inside d_data: likewise); dropped[e], the packets that left;
 *                           retained[e], the packets the slot holds now.  A run that does not fit makes the slot drop,
 *                           from the front, the fewest packets such that what remains is at most half of each capacity
 *                           and leaves room for the run; the rest moves to the front of the region.  Enqueues on
 *                           `stream` and waits for it once: 40 B per entry and 12 B per new packet come back for the
 *                           host planner, and the caller's arrays are free when it returns.  VBM_EINVAL, with nothing
 *                           changed: an id out of range or listed twice, a negative count, a slot without a class.
 *   vbm_live_store_restart  the listed slots (distinct) are empty and fresh; classes [n] (host) for a store of a mixed
 *                           decoder, which sets each slot's class until its next restart, and NULL for any other.
 *                           Only enqueues.
 *   vbm_live_store_state    first_sample, totals, packets, bytes [nstreams] and trims [2] (trims the packet cap made,
 *                           trims the byte cap made), from the host's mirror; any may be NULL.
 *   vbm_live_store_snapshot the retained packets of all streams as a compact index and CSR in host arrays, the form
 *                           vbm_host_ogg_cut_ranges takes: first [nstreams + 1]; status, begin, out_end [P]; totals
 *                           [nstreams]; data, offsets [P + 1], with P and the bytes summed from vbm_live_store_state.
 *                           Waits for `stream`.
 * Calls on one store (append, restart, ranges, cut, snapshot) are ordered by the caller on one stream.
 * vbm_host_live_store_*: the CPU twin over host memory, from the same source (csrc/live_store.h): no device and no
 * decoder, only the setup and the rate.  Its append refuses offsets that are no CSR with VBM_EINVAL for the whole call.
 * A host store in a device call, or the reverse, is VBM_EINVAL. */
#define VBM_LIVE_EBIG (-1004)
int  vbm_live_store_create(vbm_range_store **st, vbm_decoder *dec, int nstreams, int max_packets, long long max_bytes);
int  vbm_live_store_create_mixed(vbm_range_store **st, vbm_decoder *dec, int nstreams, int max_packets,
                                 long long max_bytes);
int  vbm_live_store_append(vbm_range_store *st, int n, const int *stream_ids, const int *run_packets,
                           const uint8_t *d_data, const long long *d_offsets, long long data_bytes,
                           const long long *d_granulepos, const uint8_t *d_eos, const uint8_t *d_gap, int *status,
                           int *dropped, int *retained, void *stream);
int  vbm_live_store_restart(vbm_range_store *st, int n, const int *stream_ids, const int *classes, void *stream);
int  vbm_live_store_state(const vbm_range_store *st, long long *first_sample, long long *totals, long long *packets,
                          long long *bytes, long long *trims);
int  vbm_live_store_snapshot(const vbm_range_store *st, long long *first, int *status, int *begin, long long *out_end,
                             long long *totals, uint8_t *data, long long *offsets, void *stream);
int  vbm_host_live_store_create(vbm_range_store **st, const vbm_decode_setup *ds, int halfrate, int nstreams,
                                int max_packets, long long max_bytes);
int  vbm_host_live_store_append(vbm_range_store *st, int n, const int *stream_ids, const int *run_packets,
                                const uint8_t *data, const long long *offsets, long long data_bytes,
                                const long long *granulepos, const uint8_t *eos, const uint8_t *gap, int *status,
                                int *dropped, int *retained);
int  vbm_host_live_store_restart(vbm_range_store *st, int n, const int *stream_ids);
int  vbm_host_live_store_state(const vbm_range_store *st, long long *first_sample, long long *totals,
                               long long *packets, long long *bytes, long long *trims);
int  vbm_host_live_store_snapshot(const vbm_range_store *st, long long *first, int *status, int *begin,
                                  long long *out_end, long long *totals, uint8_t *data, long long *offsets);

/* ---- test instrumentation --------------------------------------------------------------------------------
 * The path is spread over several internal HIP streams; events order them.  These calls make a missing edge show
 * deterministically (tests/test_ordering_gpu.py); they change timing and scratch contents only, never results.
 *   vbm_debug_set_delay      a kernel that spins for `usec` microseconds (<= 100000) is put in front of the work at
 *                            every point of the host code whose bit is set in `mask` (points: csrc/vbm_internal.h,
 *                            enum vbm_delay_point); process-wide; usec = 0 switches it off
 *   vbm_debug_poison_workspace  fills the scratch arrays of encoder workspace w (-1: all) with `byte`, device idle
 *   vbm_debug_poison_frontend   the same for the front end's block buffers, search spectra and round lists
 *   vbm_debug_frontend_buffers  where every stream's samples lie, once the front end's stream has drained: base, parity,
 *                            pcm_current [S]; shift [2 + S]: the compaction list's count (0 between rounds), the count of
 *                            the newest round that shifted, that round's list; live (may be NULL) [S][ch][live_stride]:
 *                            the pcm_current samples of every channel buffer from the stream's origin on
 * Some launchers take another kernel, or another slicing of the same kernel, once a batch is large (csrc/batch.h,
 * "kernel variants chosen by batch size").  vbm_debug_batch_variants says which forms a batch of `nsb` stream-blocks of
 * `ch` channels takes, from the launchers' own predicates; block_mode 0..3, n = blocksize / 2, few: the batch is a
 * device-built round's (small whatever its launch bound).  Pure host arithmetic: no device, no handle.  Bits:
 *   0  floor fit by the lane-per-channel-block kernel (else the cooperative one)
 *   1  coarse slices of the bin range in offset-and-mix (never for block_mode 0, which is not sliced)
 *   2  coarse slices of the floor render
 *   3  coarse slices of the residue partitions (at most 32 per submap, else at most 256)
 *   4  offset-and-mix leaves the floor fit's input words itself (no separate pass); decided when a batch is
 *      configured, so for a slice of a batch or a round's batch the size to ask about is the whole batch's, few = 0 */
int vbm_debug_set_delay(unsigned mask, int usec);
unsigned vbm_debug_batch_variants(int block_mode, int n, int ch, int nsb, int few);
int vbm_debug_poison_workspace(vbm_encoder *enc, int w, int byte);
int vbm_debug_poison_frontend(vbm_frontend *fe, int byte);
int vbm_debug_frontend_buffers(vbm_frontend *fe, int *base, int *parity, int *pcm_current, int *shift, float *live,
                               long long live_stride);

#ifdef __cplusplus
}
#endif
#endif /* VORBIS_MI355X_H */
