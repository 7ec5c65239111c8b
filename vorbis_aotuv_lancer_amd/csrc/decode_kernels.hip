// Decode kernels for gfx950 (MI355X): Vorbis audio packets -> PCM, one row per stream.
//
//   k_unpack      one lane per packet: vbmd_unpack (decode.h, the same source as vbm_host_unpack_packet) — mode,
//                 floor 1 Y list, residue VQ — and the row lists by block size (device-side, no host round trip)
//   k_spectrum    one workgroup per row, wide over bins: floor line (closed form of render_line, lib/floor1.c:368),
//                 inverse coupling in reverse step order (mapping0_inverse, lib/mapping0.c:1381 scalar branch), and
//                 spectrum = residue * FLOOR1_fromdB_LOOKUP[floor index]
//   k_imdct*      mdct_backward (lib/mdct.c:1276, scalar branch at :1537) with the butterflies and bit-reverse of the
//                 forward kernels (mdct_butterflies.h), one wavefront per 512-complex group
//   k_overlap     one workgroup per row: vorbis_synthesis_blockin's overlap-add and copy (lib/block.c:897-1166, scalar
//                 branches), granulepos trimming, vorbis_synthesis_pcmout + _read of everything that became final
//
// Runs (vbm_synthesis_runs): rows are runs of consecutive packets of one stream.  k_unpack_csr addresses the packets
// through CSR offsets; k_spectrum and k_imdct* are the same launches; the serial part of blockin moves into a planning
// pass and the overlap-add reads the previous packet's IMDCT row instead of the stream's tail:
//   k_run_plan       one lane per run: walks its rows in order -> per row lW, previous valid row (or the carried
//                    tail), begin/end (k_overlap's granulepos bookkeeping) and the output offset; the run's final
//                    prevW / granulepos / sample count and its total samples
//   k_overlap_runs   one workgroup per row: k_overlap's overlap-add expression into the run's PCM at the planned offset
//   k_run_commit     one workgroup per run: the last valid row's second half -> the stream's tail (a separate launch:
//                    the first row of a run reads the tail that this writes)
//
// Ranges (vbm_synthesis_ranges): rows are pieces of a range store's streams, each a pre-roll packet and the packets
// after it.  k_range_rows maps rows to store packets, k_unpack_rows unpacks them from the store, k_spectrum and
// k_imdct* are the same launches, k_range_plan writes k_run_plan's entries from the store's index and k_overlap_runs
// runs unchanged.  No stream state is read or written.  On a mixed decoder k_range_rows<true> also writes each row's
// class (its piece's, from the piece table) into the rcls column, and the rest of the chain is the <MX = true> one.
//
// Half rate (vbm_decoder_create_halfrate; the reference's vorbis_synthesis_halfrate, lib/synthesis.c:166-179): unpack and
// spectrum are the same launches at the full block size; k_imdct<blocksizes[W] / 2> transforms the lower half of each
// spectrum (128 .. 2048 points) and k_overlap<1>, k_run_plan<1>, k_overlap_runs<1> and k_run_commit<1> are the overlap
// kernels with every size halved.  A full-rate decoder launches the <0> instantiations, in which every shift is by zero.
//
// Mixed decoders (vbm_decoder_create_mixed): the rows of one call may belong to different header classes.  Every kernel
// that reads the setup is a template on MX: the <false> instantiation is the single-class kernel, with the decoder's one
// setup and rows of `channels` channels; the <true> one takes its row's setup and blob from the class table
// (vbmd_mixed: by the row's class, or in k_run_plan / k_run_commit by the stream's) and addresses rows of M.CH channels
// and `half` = max_blocksize / 2 bins, of which a row uses its class's.  The block lists are then one per transform size
// (size_index) and hold blocks row * CH + c, and the windows come from the per-size tables.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode.h"
#include "decode_kernels.h"
#include "mdct_butterflies.h"

namespace {

using namespace vbm_mdct;

constexpr int IM_WAVES = 4;

// list of a block size in a mixed decoder: 256 -> 0 .. 4096 -> 4
__device__ __forceinline__ int size_index(int blocksize) { return 23 - __clz(blocksize); }

template <bool MX>
__device__ __forceinline__ const vbmd_setup *setup_of(const vbmd_setup *s, const vbmd_mixed &M, int cls)
{
    return MX ? M.table[cls].s : s;
}

// Row k of every unpack kernel: vbmd_unpack of its bytes, its status, and its entry in the block lists.  Single class:
// the row joins list W.  Mixed: its channels join the list of its transform size as blocks k * CH + c.  Out: the call
// has a status_out of the caller's beside the decoder's own status.
template <bool MX, int Copy, bool Out = true>
__device__ __forceinline__ void unpack_row(const vbmd_setup *__restrict__ s, const uint8_t *__restrict__ blob,
                                           const vbmd_mixed &M, int k, int nsb, const uint8_t *pkt, long nb,
                                           int *__restrict__ info, int *__restrict__ fit, int *__restrict__ flags,
                                           float *__restrict__ res, long half, uint8_t *__restrict__ cls,
                                           int *__restrict__ status, int *__restrict__ status_out,
                                           int *__restrict__ lists, int *__restrict__ counts)
{
    if (MX) {
        const vbmd_class &c = M.table[M.rcls[k]];
        s = c.s;
        blob = c.blob;
    }
    const int ch = s->channels, CH = MX ? M.CH : ch;
    const long cls_bytes = MX ? M.cls_bytes : s->max_classes;
    // an instantiation of vbmd_unpack per kernel (decode.h): as a shared out-of-line function it costs each kernel
    // 75 more VGPRs and half its occupancy
    const int st = vbmd_unpack<MX ? 3 + Copy : Copy>(*s, blob, pkt, nb, info + 4 * k, fit + (long)k * CH * VBMD_POSTS,
                                                     flags + (long)k * CH, res + (long)k * CH * half, half,
                                                     cls + (long)k * cls_bytes);
    status[k] = st;
    if (Out) status_out[k] = st;
    if (st != 0) return;
    const int W = info[4 * k + 1];
    if (MX) {
        const int z = size_index(s->blocksizes[W]);
        const int pos = atomicAdd(&counts[z], ch);
        for (int c = 0; c < ch; c++) lists[z * M.list_stride + pos + c] = k * CH + c;
    } else {
        const int pos = atomicAdd(&counts[W], 1);
        lists[(long)W * nsb + pos] = k;
    }
}

template <bool MX>
__global__ __launch_bounds__(64)
void k_unpack(const vbmd_setup *__restrict__ s, const uint8_t *__restrict__ blob, vbmd_mixed M, int nsb,
              const uint8_t *__restrict__ packets, long stride, const int *__restrict__ nbytes, int *__restrict__ info,
              int *__restrict__ fit, int *__restrict__ flags, float *__restrict__ res, long half,
              uint8_t *__restrict__ cls, int *__restrict__ status, int *__restrict__ status_out,
              int *__restrict__ lists, int *__restrict__ counts)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsb) return;
    long nb = nbytes[k];
    if (nb > stride) nb = stride;          // never past the row's storage either
    if (nb < 0) nb = 0;
    unpack_row<MX, 0>(s, blob, M, k, nsb, packets + (long)k * stride, nb, info, fit, flags, res, half, cls, status,
                      status_out, lists, counts);
}

// k_unpack over CSR rows: packet k is data[offsets[k] .. offsets[k+1]), clamped to [0, data_bytes)
template <bool MX>
__global__ __launch_bounds__(64)
void k_unpack_csr(const vbmd_setup *__restrict__ s, const uint8_t *__restrict__ blob, vbmd_mixed M, int nsb,
                  const uint8_t *__restrict__ data, const long long *__restrict__ offsets, long long data_bytes,
                  int *__restrict__ info, int *__restrict__ fit, int *__restrict__ flags, float *__restrict__ res,
                  long half, uint8_t *__restrict__ cls, int *__restrict__ status, int *__restrict__ status_out,
                  int *__restrict__ lists, int *__restrict__ counts)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsb) return;
    long long b = offsets[k], e = offsets[k + 1];
    b = b < 0 ? 0 : b > data_bytes ? data_bytes : b;
    e = e < b ? b : e > data_bytes ? data_bytes : e;
    unpack_row<MX, 1>(s, blob, M, k, nsb, data + b, (long)(e - b), info, fit, flags, res, half, cls, status, status_out,
                      lists, counts);
}

// floor index at bin j of the used-post polyline (segx strictly ascending, segx[0] = 0): render_line's Bresenham
// walk in closed form — after k steps from x0 the error term has wrapped floor(k*ady'/adx) times
__device__ __forceinline__ int floor_at(const int *segx, const int *segy, int m, int j)
{
    int lo = 0, hi = m;                     // largest i with segx[i] <= j
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (segx[mid] <= j) lo = mid;
        else hi = mid;
    }
    if (lo == m - 1) return segy[lo];
    const int x0 = segx[lo], x1 = segx[lo + 1], y0 = segy[lo], y1 = segy[lo + 1];
    const int dy = y1 - y0, adx = x1 - x0;
    const int ady = dy < 0 ? -dy : dy;
    const int base = dy / adx;
    const int rem = ady - (base < 0 ? -base : base) * adx;
    const int kx = j - x0;
    const int wraps = (kx * rem) / adx;
    return y0 + kx * base + (dy < 0 ? -wraps : wraps);
}

template <bool MX>
__global__ __launch_bounds__(256)
void k_spectrum(const vbmd_setup *__restrict__ s, vbmd_mixed M, int nsb, const int *__restrict__ status,
                const int *__restrict__ info,
                const int *__restrict__ fit, const int *__restrict__ flags, const float *__restrict__ res,
                const float *__restrict__ fromdB, float *__restrict__ spec, int *__restrict__ findex, long half)
{
    __shared__ int segx[VBMD_MAXCH][VBMD_POSTS + 1], segy[VBMD_MAXCH][VBMD_POSTS + 1], nseg[VBMD_MAXCH];
    __shared__ int s_flags[VBMD_MAXCH];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (MX) s = M.table[M.rcls[row]].s;
    const int ch = s->channels, CH = MX ? M.CH : ch;
    const long rbase = (long)row * CH * half;
    if (status[row] != 0) {
        for (long i = tid; i < ch * half; i += blockDim.x) {
            if (spec) spec[rbase + i] = 0.f;
            if (findex) findex[rbase + i] = 0;
        }
        return;
    }
    const int mode = info[4 * row], W = info[4 * row + 1];
    const int n = s->blocksizes[W] >> 1;
    const vbmd_mapping &m = s->map[s->mode_mapping[mode]];
    if (tid < ch) {
        const int c = tid;
        const int fl = flags[(long)row * CH + c];
        s_flags[c] = fl;
        int cnt = 0;
        if (fl & 1) {
            const vbmd_floor &f = s->floor[m.floorsub[m.mux[c]]];
            const int *fv = fit + ((long)row * CH + c) * VBMD_POSTS;
            int ly = fv[0] * f.mult;
            ly = ly < 0 ? 0 : ly > 255 ? 255 : ly;
            segx[c][0] = 0;
            segy[c][0] = ly;
            cnt = 1;
            for (int j = 1; j < f.posts; j++) {
                const int cur = f.fwd[j];
                int hy = fv[cur] & 0x7fff;
                if (hy != fv[cur]) continue;
                hy *= f.mult;
                segx[c][cnt] = f.postlist[cur];
                segy[c][cnt] = hy < 0 ? 0 : hy > 255 ? 255 : hy;
                cnt++;
            }
        }
        nseg[c] = cnt;
    }
    __syncthreads();
    for (int j = tid; j < half; j += blockDim.x) {
        if (j >= n) {
            for (int c = 0; c < ch; c++) {
                if (spec) spec[rbase + c * half + j] = 0.f;
                if (findex) findex[rbase + c * half + j] = 0;
            }
            continue;
        }
        if (findex) {
            for (int c = 0; c < ch; c++)
                findex[rbase + c * half + j] = (s_flags[c] & 1) ? floor_at(segx[c], segy[c], nseg[c], j) : 0;
            continue;
        }
        float v[VBMD_MAXCH];
        for (int c = 0; c < ch; c++) v[c] = res[rbase + c * half + j];
        for (int i = m.steps - 1; i >= 0; i--) {
            const float mag = v[m.mag[i]], ang = v[m.ang[i]];
            float pm, pa;
            if (mag > 0) {
                if (ang > 0) { pm = mag; pa = mag - ang; }
                else { pa = mag; pm = mag + ang; }
            } else {
                if (ang > 0) { pm = mag; pa = mag + ang; }
                else { pa = mag; pm = mag - ang; }
            }
            v[m.mag[i]] = pm;
            v[m.ang[i]] = pa;
        }
        for (int c = 0; c < ch; c++)
            spec[rbase + c * half + j] =
                (s_flags[c] & 1) ? v[c] * fromdB[min(max(floor_at(segx[c], segy[c], nseg[c], j), 0), 255)] : 0.f;
    }
}

// mdct_backward's first rotation (lib/mdct.c:1537-1566) for complex element p of an N-point block -> the input of
// mdct_butterflies (out + n2)
template <int N>
__device__ __forceinline__ float2 backward_rotate(const float *__restrict__ in, const float *T, int p)
{
    constexpr int n2 = N / 2, n4 = N / 4, n8 = N / 8;
    float2 r;
    if (p < n8) {
        const int q = n8 - 1 - p, a = n2 - 1 - 4 * q, t = n4 + 2 * q;
        r.x = -in[a] * T[t + 1] - in[a - 2] * T[t];
        r.y = in[a - 2] * T[t + 1] - in[a] * T[t];
    } else {
        const int q = p - n8, c = n2 - 4 - 4 * q, t = n4 - 2 * q - 2;
        r.x = in[c] * T[t + 1] + in[c + 2] * T[t];
        r.y = in[c] * T[t] - in[c + 2] * T[t + 1];
    }
    return r;
}

// the second rotation and the unfold (lib/mdct.c:1571-1626) of w pair u: out[C-1-u] = A, out[C+u] = -A,
// out[3C-1-u] = B, out[3C+u] = B
__device__ __forceinline__ void backward_post(float2 w, float2 T, float &A, float &B)
{
    A = w.x * T.y - w.y * T.x;
    B = -(w.x * T.x + w.y * T.y);
}

__device__ __forceinline__ void store_rev4(float *o, const float *v)   // o[0..3] = v[3], v[2], v[1], v[0]
{
    *reinterpret_cast<float4 *>(o) = make_float4(v[3], v[2], v[1], v[0]);
}

// entry blk of a transform's list -> its block, row * channels + channel, of the spectrum and IMDCT buffers
template <bool MX>
__device__ __forceinline__ long block_of(const int *__restrict__ list, long blk, int ch)
{
    return MX ? (long)list[blk] : (long)list[blk / ch] * ch + blk % ch;
}

// one wavefront per 512-complex group (BPG blocks of N = 128 .. 2048; 128 only in a half-rate decoder, whose transform
// of a 256-sample block it is); blocks b of the row list of this block size.  Reads in[0, N/2) of each block's `half`
// bins and writes N floats of its n1-float output row.  MX: the list holds the blocks themselves (row * CH + channel),
// *count of them, so a group may hold blocks of rows of different classes; a size with no blocks ends at once.
template <int N, bool MX>
__global__ __launch_bounds__(64 * IM_WAVES)
void k_imdct(const float *__restrict__ spec, float *__restrict__ out, const int *__restrict__ list,
             const int *__restrict__ count, int ch, long half, long n1, const float *__restrict__ trig_g)
{
    constexpr int C = N / 4, BPG = 512 / C, NTRIG = N + N / 4;
    constexpr int LOG2C = (N == 2048) ? 9 : (N == 1024) ? 8 : (N == 512) ? 7 : (N == 256) ? 6 : 5;
    __shared__ __attribute__((aligned(16))) float s_trig[NTRIG];
    __shared__ __attribute__((aligned(16))) float2 s_x[IM_WAVES][SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (MX && *count == 0) return;
    for (int i = tid; i < NTRIG; i += blockDim.x) s_trig[i] = trig_g[i];
    __syncthreads();
    const long nblocks = MX ? (long)(*count) : (long)(*count) * ch;
    const long ngroups = (nblocks + BPG - 1) / BPG;
    float2 *sx = s_x[wave];
    for (long group = (long)blockIdx.x * IM_WAVES + wave; group < ngroups; group += (long)gridDim.x * IM_WAVES) {
        float2 c[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int P = lane + 64 * k, b = P / C, p = P % C;
            const long blk = group * BPG + b;
            if (blk < nblocks) {
                const float *in = spec + block_of<MX>(list, blk, ch) * half;
                c[k] = backward_rotate<N>(in, s_trig, p);
            } else {
                c[k] = make_float2(0.f, 0.f);
            }
        }
        radix_rounds<LOG2C>(c, sx, s_trig, lane);
        {
            constexpr int HALFC = C / 2;
            const int U0 = 4 * lane, b = U0 / HALFC, u0 = U0 % HALFC;
            const long blk = group * BPG + b;
            float a0[4], a1[4], b0[4], b1[4];   // A/B of pair u (0) and of pair C-1-u (1)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int u = u0 + r;
                int s0, s1;
                VBM_MDCT_BITREV_SLOTS(LOG2C, C, u, s0, s1);
                const float2 X0 = sx[slot_addr(b * C + s0)], X1 = sx[slot_addr(b * C + s1)];
                const float2 T = *reinterpret_cast<const float2 *>(s_trig + N + 2 * u);
                float2 wA, wB;
                VBM_MDCT_BITREV_PAIR(X0, X1, T, wA, wB);
                backward_post(wA, *reinterpret_cast<const float2 *>(s_trig + N / 2 + 2 * u), a0[r], b0[r]);
                backward_post(wB, *reinterpret_cast<const float2 *>(s_trig + N / 2 + 2 * (C - 1 - u)), a1[r], b1[r]);
            }
            if (blk < nblocks) {
                float *o = out + block_of<MX>(list, blk, ch) * n1;
                float na0[4], na1[4];
#pragma unroll
                for (int r = 0; r < 4; r++) { na0[r] = -a0[r]; na1[r] = -a1[r]; }
                store_rev4(o + C - 4 - u0, a0);                                   // out[C-1-u]   = A(u)
                *reinterpret_cast<float4 *>(o + C + u0) = make_float4(na0[0], na0[1], na0[2], na0[3]);   // out[C+u]
                store_rev4(o + 3 * C - 4 - u0, b0);                               // out[3C-1-u]  = B(u)
                *reinterpret_cast<float4 *>(o + 3 * C + u0) = make_float4(b0[0], b0[1], b0[2], b0[3]);  // out[3C+u]
                *reinterpret_cast<float4 *>(o + u0) = make_float4(a1[0], a1[1], a1[2], a1[3]);           // out[u] = A(C-1-u)
                store_rev4(o + 2 * C - 4 - u0, na1);                              // out[2C-1-u] = -A(C-1-u)
                *reinterpret_cast<float4 *>(o + 2 * C + u0) = make_float4(b1[0], b1[1], b1[2], b1[3]);  // out[2C+u]
                store_rev4(o + 4 * C - 4 - u0, b1);                               // out[4C-1-u] = B(C-1-u)
            }
        }
        wave_lds_sync();
    }
}

// 4096-point blocks: one wavefront per block, two 512-complex halves (as k_window_mdct_4096)
template <bool MX>
__global__ __launch_bounds__(64 * IM_WAVES)
void k_imdct_4096(const float *__restrict__ spec, float *__restrict__ out, const int *__restrict__ list,
                  const int *__restrict__ count, int ch, long half, long n1, const float *__restrict__ trig_g)
{
    constexpr int N = 4096, C = 1024, NTRIG = N + N / 4;
    __shared__ __attribute__((aligned(16))) float s_trig[NTRIG];
    __shared__ __attribute__((aligned(16))) float2 s_x[IM_WAVES][2][SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (MX && *count == 0) return;
    for (int i = tid; i < NTRIG; i += blockDim.x) s_trig[i] = trig_g[i];
    __syncthreads();
    const long nblocks = MX ? (long)(*count) : (long)(*count) * ch;
    float2 *sx0 = s_x[wave][0], *sx1 = s_x[wave][1];
#define SLOT(m) (((m) < 512 ? sx0 : sx1)[slot_addr((m) & 511)])
    for (long blk = (long)blockIdx.x * IM_WAVES + wave; blk < nblocks; blk += (long)gridDim.x * IM_WAVES) {
        const long block = block_of<MX>(list, blk, ch);
        const float *in = spec + block * half;
        float2 c0[8], c1[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            c0[k] = backward_rotate<N>(in, s_trig, lane + 64 * k);
            c1[k] = backward_rotate<N>(in, s_trig, lane + 64 * k + 512);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int t = 511 - (lane + 64 * k);
            bfly(c0[k], c1[k], *reinterpret_cast<const float2 *>(s_trig + 4 * t));
        }
        radix_rounds<10>(c0, sx0, s_trig, lane);
        radix_rounds<10>(c1, sx1, s_trig, lane);
        float *o = out + block * n1;
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const int u0 = 4 * lane + 256 * pass;
            float a0[4], a1[4], b0[4], b1[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int u = u0 + r;
                int s0, s1;
                VBM_MDCT_BITREV_SLOTS(10, C, u, s0, s1);
                const float2 X0 = SLOT(s0), X1 = SLOT(s1);
                const float2 T = *reinterpret_cast<const float2 *>(s_trig + N + 2 * u);
                float2 wA, wB;
                VBM_MDCT_BITREV_PAIR(X0, X1, T, wA, wB);
                backward_post(wA, *reinterpret_cast<const float2 *>(s_trig + N / 2 + 2 * u), a0[r], b0[r]);
                backward_post(wB, *reinterpret_cast<const float2 *>(s_trig + N / 2 + 2 * (C - 1 - u)), a1[r], b1[r]);
            }
            float na0[4], na1[4];
#pragma unroll
            for (int r = 0; r < 4; r++) { na0[r] = -a0[r]; na1[r] = -a1[r]; }
            store_rev4(o + C - 4 - u0, a0);
            *reinterpret_cast<float4 *>(o + C + u0) = make_float4(na0[0], na0[1], na0[2], na0[3]);
            store_rev4(o + 3 * C - 4 - u0, b0);
            *reinterpret_cast<float4 *>(o + 3 * C + u0) = make_float4(b0[0], b0[1], b0[2], b0[3]);
            *reinterpret_cast<float4 *>(o + u0) = make_float4(a1[0], a1[1], a1[2], a1[3]);
            store_rev4(o + 2 * C - 4 - u0, na1);
            *reinterpret_cast<float4 *>(o + 2 * C + u0) = make_float4(b1[0], b1[1], b1[2], b1[3]);
            store_rev4(o + 4 * C - 4 - u0, b1);
        }
        wave_lds_sync();
    }
#undef SLOT
}

// HS: 0, or 1 in a half-rate decoder (lib/block.c:897-1166 with hs = 1): every size is that of the halved block, n1 the
// IMDCT row of blocksizes[1] >> HS floats, `half` the tail and PCM row of blocksizes[1] >> (1 + HS), win0 / win1 the
// windows of the halved sizes.  MX: `half` is the tail and PCM row of the decoder's largest block, of which the row's
// class uses the front, and win0 / win1 are the class's own, from the per-size tables.
template <int HS, bool MX>
__global__ __launch_bounds__(256)
void k_overlap(const vbmd_setup *__restrict__ s, vbmd_mixed M, int nsb, const int *__restrict__ ids,
               const int *__restrict__ status, const int *__restrict__ info, const float *__restrict__ imdct, long n1,
               const float *__restrict__ win0, const float *__restrict__ win1,
               const long long *__restrict__ granulepos, const uint8_t *__restrict__ eos,
               float *__restrict__ tail, int *__restrict__ prevW, long long *__restrict__ st_gp,
               long long *__restrict__ st_sc, float *__restrict__ pcm, int *__restrict__ samples, long half)
{
    const int row = blockIdx.x, tid = threadIdx.x;
    if (status[row] != 0) {
        if (tid == 0) samples[row] = 0;
        return;
    }
    if (MX) s = M.table[M.rcls[row]].s;
    const int ch = s->channels, CH = MX ? M.CH : ch, sid = ids[row];
    const int W = info[4 * row + 1], lW = prevW[sid];
    const int bs0 = s->blocksizes[0], bs1 = s->blocksizes[1];
    const int n = s->blocksizes[W] >> (1 + HS), n0 = bs0 >> (1 + HS), nh1 = bs1 >> (1 + HS);
    if (MX) {
        win0 = M.win[size_index(bs0)];
        win1 = M.win[size_index(bs1)];
    }
    // vorbis_synthesis_blockin: what becomes final, and the granulepos bookkeeping
    long long sc = st_sc[sid], gp = st_gp[sid];
    const long long vgp = granulepos ? granulepos[row] : -1;
    const int eof = eos ? eos[row] : 0;
    long begin, end;
    vbmd_blockin<HS>(s->blocksizes, lW, W, vgp, eof, sc, gp, begin, end);
    for (int c = 0; c < ch; c++) {
        const float *p = imdct + ((long)row * CH + c) * n1;
        float *t = tail + ((long)sid * CH + c) * half;
        float *o = pcm + ((long)row * CH + c) * half;
        for (long i = begin + tid; i < end; i += blockDim.x) {
            float v;
            if (lW == 1 && W == 1) {
                v = t[i] * win1[nh1 - i - 1] + p[i] * win1[i];
            } else if (lW == 1) {
                const long off = nh1 / 2 - n0 / 2;
                if (i < off) v = t[i];
                else { const long k = i - off; v = t[i] * win0[n0 - k - 1] + p[k] * win0[k]; }
            } else if (W == 1) {
                const long off = nh1 / 2 - n0 / 2;
                if (i < n0) v = t[i] * win0[n0 - i - 1] + p[off + i] * win0[i];
                else v = p[off + i];
            } else {
                v = t[i] * win0[n0 - i - 1] + p[i] * win0[i];
            }
            o[i - begin] = v;
        }
        __syncthreads();                    // every read of the old tail is done
        for (int i = tid; i < n; i += blockDim.x) t[i] = p[n + i];
    }
    __syncthreads();
    if (tid == 0) {
        samples[row] = (int)(end - begin);
        prevW[sid] = W;
        st_gp[sid] = gp;
        st_sc[sid] = sc;
    }
}

// One lane per run.  runtab: ids[nruns], then the run starts [nruns + 1] (rows are the runs concatenated).  Per row:
// plan[k] = {run, previous valid row of the run (-1: the stream's tail), lW, begin, end, output offset}, and samples[k].
// The run's final prevW / granulepos / sample count go straight to the stream state: no kernel of this call reads
// them after this one.  run_last[r]: the run's last valid row (-1: none), for k_run_commit.
template <int HS, bool MX>
__global__ __launch_bounds__(64)
void k_run_plan(const vbmd_setup *__restrict__ s, vbmd_mixed M, int nruns, const int *__restrict__ runtab,
                const int *__restrict__ status, const int *__restrict__ info,
                const long long *__restrict__ granulepos, const uint8_t *__restrict__ eos,
                const uint8_t *__restrict__ gap, int *__restrict__ prevW,
                long long *__restrict__ st_gp, long long *__restrict__ st_sc, int *__restrict__ plan,
                int *__restrict__ samples, int *__restrict__ run_samples, int *__restrict__ run_last)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const int sid = runtab[r], k0 = runtab[nruns + r], k1 = runtab[nruns + r + 1];
    if (MX) s = M.table[M.scls[sid]].s;
    int lW = prevW[sid], prev = -1, off = 0;
    long long sc = st_sc[sid], gp = st_gp[sid];
    for (int k = k0; k < k1; k++) {
        int *pl = plan + 6 * (long)k;
        if (gap && gap[k]) sc = gp = -1;            // packets were lost: lib/block.c:911-915; an error row hands it on
        if (status[k] != 0) {
            samples[k] = 0;
            continue;
        }
        const int W = info[4 * k + 1];
        const long long vgp = granulepos ? granulepos[k] : -1;
        const int eof = eos ? eos[k] : 0;
        long begin, end;
        vbmd_blockin<HS>(s->blocksizes, lW, W, vgp, eof, sc, gp, begin, end);   // k_overlap's bookkeeping
        pl[0] = r;
        pl[1] = prev;
        pl[2] = lW;
        pl[3] = (int)begin;
        pl[4] = (int)end;
        pl[5] = off;
        samples[k] = (int)(end - begin);
        off += (int)(end - begin);
        prev = k;
        lW = W;
    }
    prevW[sid] = lW;
    st_gp[sid] = gp;
    st_sc[sid] = sc;
    run_samples[r] = off;
    run_last[r] = prev;
}

// One workgroup per row: k_overlap's overlap-add, term for term, with the tail read from the previous valid row's
// IMDCT output (its second half, which is what k_overlap's tail copy would hold) or, for a run's first valid row,
// from the stream's tail.  Output: the run's PCM [nruns][ch][pcm_stride] at the planned offset.
template <int HS, bool MX>
__global__ __launch_bounds__(256)
void k_overlap_runs(const vbmd_setup *__restrict__ s, vbmd_mixed M, const int *__restrict__ runtab,
                    const int *__restrict__ status, const int *__restrict__ info, const int *__restrict__ plan,
                    const float *__restrict__ imdct, long n1,
                    const float *__restrict__ win0, const float *__restrict__ win1, const float *__restrict__ tail,
                    float *__restrict__ pcm, long pcm_stride, long half)
{
    const int row = blockIdx.x, tid = threadIdx.x;
    if (status[row] != 0) return;
    const int *pl = plan + 6 * (long)row;
    const int run = pl[0], prev = pl[1], lW = pl[2];
    const long begin = pl[3], end = pl[4], off = pl[5];
    if (end <= begin) return;                   // lW < 0 (end = 0) included
    if (MX) s = M.table[M.rcls[row]].s;
    const int ch = s->channels, CH = MX ? M.CH : ch, sid = runtab[run];
    const int W = info[4 * row + 1];
    const int bs0 = s->blocksizes[0], bs1 = s->blocksizes[1];
    const int n0 = bs0 >> (1 + HS), nh1 = bs1 >> (1 + HS);
    if (MX) {
        win0 = M.win[size_index(bs0)];
        win1 = M.win[size_index(bs1)];
    }
    for (int c = 0; c < ch; c++) {
        const float *p = imdct + ((long)row * CH + c) * n1;
        const float *t = prev >= 0 ? imdct + ((long)prev * CH + c) * n1 + (s->blocksizes[lW] >> (1 + HS))
                                   : tail + ((long)sid * CH + c) * half;
        float *o = pcm + ((long)run * CH + c) * pcm_stride + off;
        for (long i = begin + tid; i < end; i += blockDim.x) {
            float v;
            if (lW == 1 && W == 1) {
                v = t[i] * win1[nh1 - i - 1] + p[i] * win1[i];
            } else if (lW == 1) {
                const long o2 = nh1 / 2 - n0 / 2;
                if (i < o2) v = t[i];
                else { const long k = i - o2; v = t[i] * win0[n0 - k - 1] + p[k] * win0[k]; }
            } else if (W == 1) {
                const long o2 = nh1 / 2 - n0 / 2;
                if (i < n0) v = t[i] * win0[n0 - i - 1] + p[o2 + i] * win0[i];
                else v = p[o2 + i];
            } else {
                v = t[i] * win0[n0 - i - 1] + p[i] * win0[i];
            }
            o[i - begin] = v;
        }
    }
}

// One workgroup per run: the second half of the run's last valid row -> the stream's tail (k_overlap's tail copy)
template <int HS, bool MX>
__global__ __launch_bounds__(256)
void k_run_commit(const vbmd_setup *__restrict__ s, vbmd_mixed M, int nruns, const int *__restrict__ runtab,
                  const int *__restrict__ run_last, const int *__restrict__ info, const float *__restrict__ imdct,
                  long n1, float *__restrict__ tail, long half)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const int last = run_last[r];
    if (last < 0) return;
    if (MX) s = M.table[M.scls[runtab[r]]].s;
    const int ch = s->channels, CH = MX ? M.CH : ch, sid = runtab[r];
    const int n = s->blocksizes[info[4 * last + 1]] >> (1 + HS);
    for (int c = 0; c < ch; c++) {
        const float *p = imdct + ((long)last * CH + c) * n1;
        float *t = tail + ((long)sid * CH + c) * half;
        for (int i = tid; i < n; i += blockDim.x) t[i] = p[n + i];
    }
}

// Ranges (vbm_synthesis_ranges).  A piece is a pre-roll packet of the store followed by `count` consecutive packets;
// its rows are contiguous in the call.  rtab: row starts [npieces + 1], then per piece {output row, pre-roll packet,
// first packet, window start (low, high 32 bits), window length}.  One lane per piece: row -> store packet.
// MX: the pieces' classes [npieces] (the class of each piece's stream, from the store's class column) lie behind the
// table, and every row of a piece gets its piece's class in rcls, the column the row kernels read.
template <bool MX>
__global__ __launch_bounds__(64)
void k_range_rows(int npieces, const int *__restrict__ rtab, int *__restrict__ rows, int *__restrict__ rcls)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npieces) return;
    const int k0 = rtab[p], k1 = rtab[p + 1];
    const int *pc = rtab + npieces + 1 + 6 * (long)p;
    rows[k0] = pc[1];
    for (int k = k0 + 1; k < k1; k++) rows[k] = pc[2] + (k - k0 - 1);
    if (MX) {
        const int c = rtab[7 * (long)npieces + 1 + p];
        for (int k = k0; k < k1; k++) rcls[k] = c;
    }
}

// k_unpack_csr with the bytes of row k taken from the store's packet rows[k]
template <bool MX>
__global__ __launch_bounds__(64)
void k_unpack_rows(const vbmd_setup *__restrict__ s, const uint8_t *__restrict__ blob, vbmd_mixed M, int nsb,
                   const int *__restrict__ rows, const uint8_t *__restrict__ data,
                   const long long *__restrict__ offsets, long long data_bytes, int *__restrict__ info,
                   int *__restrict__ fit, int *__restrict__ flags, float *__restrict__ res, long half,
                   uint8_t *__restrict__ cls, int *__restrict__ status, int *__restrict__ lists,
                   int *__restrict__ counts)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsb) return;
    const long j = rows[k];
    long long b = offsets[j], e = offsets[j + 1];
    b = b < 0 ? 0 : b > data_bytes ? data_bytes : b;
    e = e < b ? b : e > data_bytes ? data_bytes : e;
    unpack_row<MX, 2, false>(s, blob, M, k, nsb, data + b, (long)(e - b), info, fit, flags, res, half, cls, status,
                             nullptr, lists, counts);
}

// One lane per piece: k_run_plan's plan entries, with begin / end / out_start from the store's index instead of the
// carried granulepos state.  The pre-roll row writes nothing (end = 0); every later valid row writes the part of
// [out_start, out_start + end - begin) that lies in the piece's window, at its offset in the range's output row.
// Its previous valid row is always inside the piece, so k_overlap_runs never reads a stream's tail, and of the piece's
// class, so the plan needs no class.
__global__ __launch_bounds__(64)
void k_range_plan(int npieces, const int *__restrict__ rtab, const int *__restrict__ rows,
                  const int *__restrict__ status, const int *__restrict__ info, const int *__restrict__ pk_begin,
                  const int *__restrict__ pk_end, const long long *__restrict__ out_start, int *__restrict__ plan)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npieces) return;
    const int k0 = rtab[p], k1 = rtab[p + 1];
    const int *pc = rtab + npieces + 1 + 6 * (long)p;
    const int r = pc[0];
    const long long ws = (long long)(((unsigned long long)(unsigned)pc[4] << 32) | (unsigned)pc[3]);
    const long long we = ws + pc[5];
    int *pl = plan + 6 * (long)k0;
    pl[0] = r;
    pl[1] = -1;
    pl[2] = -1;
    pl[3] = pl[4] = pl[5] = 0;
    int prev = k0, lW = info[4 * k0 + 1];
    for (int k = k0 + 1; k < k1; k++) {
        if (status[k] != 0) continue;
        const int j = rows[k];
        const long long o = out_start[j], b = pk_begin[j], n = pk_end[j] - b;
        const long long lo = o > ws ? o : ws, hi = o + n < we ? o + n : we;
        pl = plan + 6 * (long)k;
        pl[0] = r;
        pl[1] = prev;
        pl[2] = lW;
        pl[3] = hi > lo ? (int)(b + lo - o) : 0;
        pl[4] = hi > lo ? (int)(b + hi - o) : 0;
        pl[5] = hi > lo ? (int)(lo - ws) : 0;
        prev = k;
        lW = info[4 * k + 1];
    }
}

// cls (vbm_decoder_bind_streams): the new class of each of the streams, written to the stream -> class map scls
__global__ void k_restart(const int *__restrict__ ids, int n, int *__restrict__ prevW, long long *__restrict__ gp,
                          long long *__restrict__ sc, const int *__restrict__ cls, int *__restrict__ scls)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (cls) scls[ids[k]] = cls[k];
    prevW[ids[k]] = -1;
    gp[ids[k]] = -1;
    sc[ids[k]] = -1;
}

__global__ void k_used(const int *__restrict__ flags, int *__restrict__ out, long n)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = (flags[k] >> 1) & 1;
}

inline int last_err() { return hipGetLastError() == hipSuccess ? 0 : -2; }

}  // namespace

// the instantiation of kernel K for the decoder of L: K<MX>, or K<HS, MX>
#define PICK_MX(K) (L.mx ? K<true> : K<false>)
#define PICK_HS_MX(K) (L.hs ? (L.mx ? K<1, true> : K<1, false>) : (L.mx ? K<0, true> : K<0, false>))

int vbmd_launch_unpack(const vbmd_launch &L, const uint8_t *packets, long stride, const int *nbytes, int *status_out,
                       hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    const auto kernel = PICK_MX(k_unpack);
    hipLaunchKernelGGL(kernel, dim3((L.nsb + 63) / 64), dim3(64), 0, q, L.s, L.blob, L.M, L.nsb, packets, stride, nbytes,
                       L.info, L.fit, L.flags, L.res, L.half, L.cls, L.status, status_out, L.lists, L.counts);
    return last_err();
}

int vbmd_launch_spectrum(const vbmd_launch &L, float *spec, int *findex, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    const auto kernel = PICK_MX(k_spectrum);
    hipLaunchKernelGGL(kernel, dim3(L.nsb), dim3(256), 0, q, L.s, L.M, L.nsb, L.status, L.info, L.fit, L.flags, L.res,
                       L.fromdB, spec, findex, L.half);
    return last_err();
}

int vbmd_launch_imdct(const vbmd_launch &L, int W, int N, const float *trig, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    const long nblocks = L.nblocks;
    const int *list = L.lists + (L.mx ? W * L.M.list_stride : (long)W * L.nsb), *count = L.counts + W;
    if (N == 4096) {
        long wgs = (nblocks + IM_WAVES - 1) / IM_WAVES;
        if (wgs > 2048) wgs = 2048;
        const auto kernel = PICK_MX(k_imdct_4096);
        hipLaunchKernelGGL(kernel, dim3((unsigned)wgs), dim3(64 * IM_WAVES), 0, q, L.spec, L.imdct, list, count, L.ch,
                           L.half, L.n1, trig);
        return last_err();
    }
    const int bpg = 2048 / N;
    long wgs = ((nblocks + bpg - 1) / bpg + IM_WAVES - 1) / IM_WAVES;
    if (wgs > 2048) wgs = 2048;
    dim3 grid((unsigned)wgs), block(64 * IM_WAVES);
#define LAUNCH(NN) \
    do { \
        const auto kernel = L.mx ? k_imdct<NN, true> : k_imdct<NN, false>; \
        hipLaunchKernelGGL(kernel, grid, block, 0, q, L.spec, L.imdct, list, count, L.ch, L.half, L.n1, trig); \
    } while (0)
    if (N == 2048) LAUNCH(2048);
    else if (N == 1024) LAUNCH(1024);
    else if (N == 512) LAUNCH(512);
    else if (N == 256) LAUNCH(256);
    else if (N == 128) LAUNCH(128);
    else return -1;
#undef LAUNCH
    return last_err();
}

int vbmd_launch_overlap(const vbmd_launch &L, const int *ids, const long long *granulepos, const uint8_t *eos,
                        float *pcm, int *samples, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    const auto kernel = PICK_HS_MX(k_overlap);
    hipLaunchKernelGGL(kernel, dim3(L.nsb), dim3(256), 0, q, L.s, L.M, L.nsb, ids, L.status, L.info, L.imdct, L.n1,
                       L.win0, L.win1, granulepos, eos, L.tail, L.prevW, L.gp, L.sc, pcm, samples, L.ohalf);
    return last_err();
}

int vbmd_launch_restart(const int *ids, int n, int *prevW, long long *gp, long long *sc, const int *cls, int *scls,
                        hipStream_t q)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_restart, dim3((n + 255) / 256), dim3(256), 0, q, ids, n, prevW, gp, sc, cls, scls);
    return last_err();
}

int vbmd_launch_used(const int *flags, int *out, long n, hipStream_t q)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_used, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, flags, out, n);
    return last_err();
}

int vbmd_launch_unpack_csr(const vbmd_launch &L, const uint8_t *data, const long long *offsets, long long data_bytes,
                           int *status_out, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    const auto kernel = PICK_MX(k_unpack_csr);
    hipLaunchKernelGGL(kernel, dim3((L.nsb + 63) / 64), dim3(64), 0, q, L.s, L.blob, L.M, L.nsb, data, offsets,
                       data_bytes, L.info, L.fit, L.flags, L.res, L.half, L.cls, L.status, status_out, L.lists,
                       L.counts);
    return last_err();
}

int vbmd_launch_runs(const vbmd_launch &L, int nruns, const int *runtab, const long long *granulepos,
                     const uint8_t *eos, const uint8_t *gap, int *plan, int *run_last, float *pcm, long pcm_stride,
                     int *run_samples, int *samples, hipStream_t q)
{
    if (nruns <= 0) return 0;
    const auto plan_kernel = PICK_HS_MX(k_run_plan);
    hipLaunchKernelGGL(plan_kernel, dim3((nruns + 63) / 64), dim3(64), 0, q, L.s, L.M, nruns, runtab, L.status, L.info,
                       granulepos, eos, gap, L.prevW, L.gp, L.sc, plan, samples, run_samples, run_last);
    if (last_err()) return -2;
    if (L.nsb > 0) {
        const auto overlap_kernel = PICK_HS_MX(k_overlap_runs);
        hipLaunchKernelGGL(overlap_kernel, dim3(L.nsb), dim3(256), 0, q, L.s, L.M, runtab, L.status, L.info, plan,
                           L.imdct, L.n1, L.win0, L.win1, L.tail, pcm, pcm_stride, L.ohalf);
        if (last_err()) return -2;
        const auto commit_kernel = PICK_HS_MX(k_run_commit);
        hipLaunchKernelGGL(commit_kernel, dim3(nruns), dim3(256), 0, q, L.s, L.M, nruns, runtab, run_last, L.info,
                           L.imdct, L.n1, L.tail, L.ohalf);
    }
    return last_err();
}

int vbmd_launch_unpack_rows(const vbmd_launch &L, int npieces, const int *rtab, int *rows, int *rcls,
                            const uint8_t *data, const long long *offsets, long long data_bytes, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    const auto rows_kernel = PICK_MX(k_range_rows);
    hipLaunchKernelGGL(rows_kernel, dim3((npieces + 63) / 64), dim3(64), 0, q, npieces, rtab, rows, rcls);
    if (last_err()) return -2;
    const auto kernel = PICK_MX(k_unpack_rows);
    hipLaunchKernelGGL(kernel, dim3((L.nsb + 63) / 64), dim3(64), 0, q, L.s, L.blob, L.M, L.nsb, rows, data, offsets,
                       data_bytes, L.info, L.fit, L.flags, L.res, L.half, L.cls, L.status, L.lists, L.counts);
    return last_err();
}

int vbmd_launch_ranges(const vbmd_launch &L, int npieces, const int *rtab, const int *rows, const int *pk_begin,
                       const int *pk_end, const long long *out_start, const int *runtab, int *plan, float *pcm,
                       long pcm_stride, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    hipLaunchKernelGGL(k_range_plan, dim3((npieces + 63) / 64), dim3(64), 0, q, npieces, rtab, rows, L.status, L.info,
                       pk_begin, pk_end, out_start, plan);
    if (last_err()) return -2;
    const auto kernel = PICK_HS_MX(k_overlap_runs);
    hipLaunchKernelGGL(kernel, dim3(L.nsb), dim3(256), 0, q, L.s, L.M, runtab, L.status, L.info, plan, L.imdct, L.n1,
                       L.win0, L.win1, L.tail, pcm, pcm_stride, L.ohalf);
    return last_err();
}

