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
// runs unchanged.  No stream state is read or written.
//
// Half rate (vbm_decoder_create_halfrate; the reference's vorbis_synthesis_halfrate, lib/synthesis.c:166-179): unpack and
// spectrum are the same launches at the full block size; k_imdct<blocksizes[W] / 2> transforms the lower half of each
// spectrum (128 .. 2048 points) and k_overlap<1>, k_run_plan<1>, k_overlap_runs<1> and k_run_commit<1> are the overlap
// kernels with every size halved.  A full-rate decoder launches the <0> instantiations, in which every shift is by zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode.h"
#include "decode_kernels.h"
#include "mdct_butterflies.h"

namespace {

using namespace vbm_mdct;

constexpr int IM_WAVES = 4;

__global__ __launch_bounds__(64)
void k_unpack(const vbmd_setup *__restrict__ s, const uint8_t *__restrict__ blob, int nsb,
              const uint8_t *__restrict__ packets, long stride, const int *__restrict__ nbytes, int *__restrict__ info,
              int *__restrict__ fit, int *__restrict__ flags, float *__restrict__ res, long half,
              uint8_t *__restrict__ cls, int *__restrict__ status, int *__restrict__ status_out,
              int *__restrict__ lists, int *__restrict__ counts)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsb) return;
    const int ch = s->channels;
    long nb = nbytes[k];
    if (nb > stride) nb = stride;          // never past the row's storage either
    if (nb < 0) nb = 0;
    const int st = vbmd_unpack(*s, blob, packets + (long)k * stride, nb, info + 4 * k, fit + (long)k * ch * VBMD_POSTS,
                               flags + (long)k * ch, res + (long)k * ch * half, half, cls + (long)k * s->max_classes);
    status[k] = st;
    status_out[k] = st;
    if (st == 0) {
        const int W = info[4 * k + 1];
        const int pos = atomicAdd(&counts[W], 1);
        lists[(long)W * nsb + pos] = k;
    }
}

// k_unpack over CSR rows: packet k is data[offsets[k] .. offsets[k+1]), clamped to [0, data_bytes)
__global__ __launch_bounds__(64)
void k_unpack_csr(const vbmd_setup *__restrict__ s, const uint8_t *__restrict__ blob, int nsb,
                  const uint8_t *__restrict__ data, const long long *__restrict__ offsets, long long data_bytes,
                  int *__restrict__ info, int *__restrict__ fit, int *__restrict__ flags, float *__restrict__ res,
                  long half, uint8_t *__restrict__ cls, int *__restrict__ status, int *__restrict__ status_out,
                  int *__restrict__ lists, int *__restrict__ counts)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsb) return;
    const int ch = s->channels;
    long long b = offsets[k], e = offsets[k + 1];
    b = b < 0 ? 0 : b > data_bytes ? data_bytes : b;
    e = e < b ? b : e > data_bytes ? data_bytes : e;
    const int st = vbmd_unpack<1>(*s, blob, data + b, (long)(e - b), info + 4 * k, fit + (long)k * ch * VBMD_POSTS,
                                  flags + (long)k * ch, res + (long)k * ch * half, half, cls + (long)k * s->max_classes);
    status[k] = st;
    status_out[k] = st;
    if (st == 0) {
        const int W = info[4 * k + 1];
        const int pos = atomicAdd(&counts[W], 1);
        lists[(long)W * nsb + pos] = k;
    }
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

__global__ __launch_bounds__(256)
void k_spectrum(const vbmd_setup *__restrict__ s, int nsb, const int *__restrict__ status, const int *__restrict__ info,
                const int *__restrict__ fit, const int *__restrict__ flags, const float *__restrict__ res,
                const float *__restrict__ fromdB, float *__restrict__ spec, int *__restrict__ findex, long half)
{
    __shared__ int segx[VBMD_MAXCH][VBMD_POSTS + 1], segy[VBMD_MAXCH][VBMD_POSTS + 1], nseg[VBMD_MAXCH];
    __shared__ int s_flags[VBMD_MAXCH];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int ch = s->channels;
    const long rbase = (long)row * ch * half;
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
        const int fl = flags[(long)row * ch + c];
        s_flags[c] = fl;
        int cnt = 0;
        if (fl & 1) {
            const vbmd_floor &f = s->floor[m.floorsub[m.mux[c]]];
            const int *fv = fit + ((long)row * ch + c) * VBMD_POSTS;
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

// one wavefront per 512-complex group (BPG blocks of N = 128 .. 2048; 128 only in a half-rate decoder, whose transform
// of a 256-sample block it is); blocks b of the row list of this block size.  Reads in[0, N/2) of each block's `half`
// bins and writes N floats of its n1-float output row.
template <int N>
__global__ __launch_bounds__(64 * IM_WAVES)
void k_imdct(const float *__restrict__ spec, float *__restrict__ out, const int *__restrict__ list,
             const int *__restrict__ count, int ch, long half, long n1, const float *__restrict__ trig_g)
{
    constexpr int C = N / 4, BPG = 512 / C, NTRIG = N + N / 4;
    constexpr int LOG2C = (N == 2048) ? 9 : (N == 1024) ? 8 : (N == 512) ? 7 : (N == 256) ? 6 : 5;
    __shared__ __attribute__((aligned(16))) float s_trig[NTRIG];
    __shared__ __attribute__((aligned(16))) float2 s_x[IM_WAVES][SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NTRIG; i += blockDim.x) s_trig[i] = trig_g[i];
    __syncthreads();
    const long nblocks = (long)(*count) * ch;
    const long ngroups = (nblocks + BPG - 1) / BPG;
    float2 *sx = s_x[wave];
    for (long group = (long)blockIdx.x * IM_WAVES + wave; group < ngroups; group += (long)gridDim.x * IM_WAVES) {
        float2 c[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int P = lane + 64 * k, b = P / C, p = P % C;
            const long blk = group * BPG + b;
            if (blk < nblocks) {
                const long row = list[blk / ch];
                const float *in = spec + (row * ch + blk % ch) * half;
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
                const long row = list[blk / ch];
                float *o = out + (row * ch + blk % ch) * n1;
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
__global__ __launch_bounds__(64 * IM_WAVES)
void k_imdct_4096(const float *__restrict__ spec, float *__restrict__ out, const int *__restrict__ list,
                  const int *__restrict__ count, int ch, long half, long n1, const float *__restrict__ trig_g)
{
    constexpr int N = 4096, C = 1024, NTRIG = N + N / 4;
    __shared__ __attribute__((aligned(16))) float s_trig[NTRIG];
    __shared__ __attribute__((aligned(16))) float2 s_x[IM_WAVES][2][SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NTRIG; i += blockDim.x) s_trig[i] = trig_g[i];
    __syncthreads();
    const long nblocks = (long)(*count) * ch;
    float2 *sx0 = s_x[wave][0], *sx1 = s_x[wave][1];
#define SLOT(m) (((m) < 512 ? sx0 : sx1)[slot_addr((m) & 511)])
    for (long blk = (long)blockIdx.x * IM_WAVES + wave; blk < nblocks; blk += (long)gridDim.x * IM_WAVES) {
        const long row = list[blk / ch];
        const float *in = spec + (row * ch + blk % ch) * half;
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
        float *o = out + (row * ch + blk % ch) * n1;
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
// windows of the halved sizes.
template <int HS>
__global__ __launch_bounds__(256)
void k_overlap(const vbmd_setup *__restrict__ s, int nsb, const int *__restrict__ ids, const int *__restrict__ status,
               const int *__restrict__ info, const float *__restrict__ imdct, long n1,
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
    const int ch = s->channels, sid = ids[row];
    const int W = info[4 * row + 1], lW = prevW[sid];
    const int bs0 = s->blocksizes[0], bs1 = s->blocksizes[1];
    const int n = s->blocksizes[W] >> (1 + HS), n0 = bs0 >> (1 + HS), nh1 = bs1 >> (1 + HS);
    // vorbis_synthesis_blockin: what becomes final, and the granulepos bookkeeping
    long long sc = st_sc[sid], gp = st_gp[sid];
    const long long vgp = granulepos ? granulepos[row] : -1;
    const int eof = eos ? eos[row] : 0;
    long begin, end;
    vbmd_blockin<HS>(s->blocksizes, lW, W, vgp, eof, sc, gp, begin, end);
    for (int c = 0; c < ch; c++) {
        const float *p = imdct + ((long)row * ch + c) * n1;
        float *t = tail + ((long)sid * ch + c) * half;
        float *o = pcm + ((long)row * ch + c) * half;
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
template <int HS>
__global__ __launch_bounds__(64)
void k_run_plan(const vbmd_setup *__restrict__ s, int nruns, const int *__restrict__ runtab,
                const int *__restrict__ status, const int *__restrict__ info,
                const long long *__restrict__ granulepos, const uint8_t *__restrict__ eos,
                const uint8_t *__restrict__ gap, int *__restrict__ prevW,
                long long *__restrict__ st_gp, long long *__restrict__ st_sc, int *__restrict__ plan,
                int *__restrict__ samples, int *__restrict__ run_samples, int *__restrict__ run_last)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const int sid = runtab[r], k0 = runtab[nruns + r], k1 = runtab[nruns + r + 1];
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
template <int HS>
__global__ __launch_bounds__(256)
void k_overlap_runs(const vbmd_setup *__restrict__ s, const int *__restrict__ runtab, const int *__restrict__ status,
                    const int *__restrict__ info, const int *__restrict__ plan, const float *__restrict__ imdct, long n1,
                    const float *__restrict__ win0, const float *__restrict__ win1, const float *__restrict__ tail,
                    float *__restrict__ pcm, long pcm_stride, long half)
{
    const int row = blockIdx.x, tid = threadIdx.x;
    if (status[row] != 0) return;
    const int *pl = plan + 6 * (long)row;
    const int run = pl[0], prev = pl[1], lW = pl[2];
    const long begin = pl[3], end = pl[4], off = pl[5];
    if (end <= begin) return;                   // lW < 0 (end = 0) included
    const int ch = s->channels, sid = runtab[run];
    const int W = info[4 * row + 1];
    const int bs0 = s->blocksizes[0], bs1 = s->blocksizes[1];
    const int n0 = bs0 >> (1 + HS), nh1 = bs1 >> (1 + HS);
    for (int c = 0; c < ch; c++) {
        const float *p = imdct + ((long)row * ch + c) * n1;
        const float *t = prev >= 0 ? imdct + ((long)prev * ch + c) * n1 + (s->blocksizes[lW] >> (1 + HS))
                                   : tail + ((long)sid * ch + c) * half;
        float *o = pcm + ((long)run * ch + c) * pcm_stride + off;
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
template <int HS>
__global__ __launch_bounds__(256)
void k_run_commit(const vbmd_setup *__restrict__ s, int nruns, const int *__restrict__ runtab,
                  const int *__restrict__ run_last, const int *__restrict__ info, const float *__restrict__ imdct,
                  long n1, float *__restrict__ tail, long half)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const int last = run_last[r];
    if (last < 0) return;
    const int ch = s->channels, sid = runtab[r];
    const int n = s->blocksizes[info[4 * last + 1]] >> (1 + HS);
    for (int c = 0; c < ch; c++) {
        const float *p = imdct + ((long)last * ch + c) * n1;
        float *t = tail + ((long)sid * ch + c) * half;
        for (int i = tid; i < n; i += blockDim.x) t[i] = p[n + i];
    }
}

// Ranges (vbm_synthesis_ranges).  A piece is a pre-roll packet of the store followed by `count` consecutive packets;
// its rows are contiguous in the call.  rtab: row starts [npieces + 1], then per piece {output row, pre-roll packet,
// first packet, window start (low, high 32 bits), window length}.  One lane per piece: row -> store packet.
__global__ __launch_bounds__(64)
void k_range_rows(int npieces, const int *__restrict__ rtab, int *__restrict__ rows)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npieces) return;
    const int k0 = rtab[p], k1 = rtab[p + 1];
    const int *pc = rtab + npieces + 1 + 6 * (long)p;
    rows[k0] = pc[1];
    for (int k = k0 + 1; k < k1; k++) rows[k] = pc[2] + (k - k0 - 1);
}

// k_unpack_csr with the bytes of row k taken from the store's packet rows[k]
__global__ __launch_bounds__(64)
void k_unpack_rows(const vbmd_setup *__restrict__ s, const uint8_t *__restrict__ blob, int nsb,
                   const int *__restrict__ rows, const uint8_t *__restrict__ data,
                   const long long *__restrict__ offsets, long long data_bytes, int *__restrict__ info,
                   int *__restrict__ fit, int *__restrict__ flags, float *__restrict__ res, long half,
                   uint8_t *__restrict__ cls, int *__restrict__ status, int *__restrict__ lists,
                   int *__restrict__ counts)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsb) return;
    const int ch = s->channels;
    const long j = rows[k];
    long long b = offsets[j], e = offsets[j + 1];
    b = b < 0 ? 0 : b > data_bytes ? data_bytes : b;
    e = e < b ? b : e > data_bytes ? data_bytes : e;
    const int st = vbmd_unpack<2>(*s, blob, data + b, (long)(e - b), info + 4 * k, fit + (long)k * ch * VBMD_POSTS,
                                  flags + (long)k * ch, res + (long)k * ch * half, half, cls + (long)k * s->max_classes);
    status[k] = st;
    if (st == 0) {
        const int W = info[4 * k + 1];
        const int pos = atomicAdd(&counts[W], 1);
        lists[(long)W * nsb + pos] = k;
    }
}

// One lane per piece: k_run_plan's plan entries, with begin / end / out_start from the store's index instead of the
// carried granulepos state.  The pre-roll row writes nothing (end = 0); every later valid row writes the part of
// [out_start, out_start + end - begin) that lies in the piece's window, at its offset in the range's output row.
// Its previous valid row is always inside the piece, so k_overlap_runs never reads a stream's tail.
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

__global__ void k_restart(const int *__restrict__ ids, int n, int *__restrict__ prevW, long long *__restrict__ gp,
                          long long *__restrict__ sc)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
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

int vbmd_launch_unpack(const vbmd_launch &L, const uint8_t *packets, long stride, const int *nbytes, int *status_out,
                       hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    hipLaunchKernelGGL(k_unpack, dim3((L.nsb + 63) / 64), dim3(64), 0, q, L.s, L.blob, L.nsb, packets, stride, nbytes,
                       L.info, L.fit, L.flags, L.res, L.half, L.cls, L.status, status_out, L.lists, L.counts);
    return last_err();
}

int vbmd_launch_spectrum(const vbmd_launch &L, float *spec, int *findex, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    hipLaunchKernelGGL(k_spectrum, dim3(L.nsb), dim3(256), 0, q, L.s, L.nsb, L.status, L.info, L.fit, L.flags, L.res,
                       L.fromdB, spec, findex, L.half);
    return last_err();
}

int vbmd_launch_imdct(const vbmd_launch &L, int W, int N, const float *trig, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    const long nblocks = (long)L.nsb * L.ch;
    const int *list = L.lists + (long)W * L.nsb, *count = L.counts + W;
    if (N == 4096) {
        long wgs = (nblocks + IM_WAVES - 1) / IM_WAVES;
        if (wgs > 2048) wgs = 2048;
        hipLaunchKernelGGL(k_imdct_4096, dim3((unsigned)wgs), dim3(64 * IM_WAVES), 0, q, L.spec, L.imdct, list, count,
                           L.ch, L.half, L.n1, trig);
        return last_err();
    }
    const int bpg = 2048 / N;
    long wgs = ((nblocks + bpg - 1) / bpg + IM_WAVES - 1) / IM_WAVES;
    if (wgs > 2048) wgs = 2048;
    dim3 grid((unsigned)wgs), block(64 * IM_WAVES);
#define LAUNCH(NN) hipLaunchKernelGGL(k_imdct<NN>, grid, block, 0, q, L.spec, L.imdct, list, count, L.ch, L.half, L.n1, trig)
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
    hipLaunchKernelGGL(L.hs ? k_overlap<1> : k_overlap<0>, dim3(L.nsb), dim3(256), 0, q, L.s, L.nsb, ids, L.status, L.info,
                       L.imdct, L.n1, L.win0, L.win1, granulepos, eos, L.tail, L.prevW, L.gp, L.sc, pcm, samples, L.ohalf);
    return last_err();
}

int vbmd_launch_restart(const int *ids, int n, int *prevW, long long *gp, long long *sc, hipStream_t q)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_restart, dim3((n + 255) / 256), dim3(256), 0, q, ids, n, prevW, gp, sc);
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
    hipLaunchKernelGGL(k_unpack_csr, dim3((L.nsb + 63) / 64), dim3(64), 0, q, L.s, L.blob, L.nsb, data, offsets,
                       data_bytes, L.info, L.fit, L.flags, L.res, L.half, L.cls, L.status, status_out, L.lists,
                       L.counts);
    return last_err();
}

int vbmd_launch_runs(const vbmd_launch &L, int nruns, const int *runtab, const long long *granulepos,
                     const uint8_t *eos, const uint8_t *gap, int *plan, int *run_last, float *pcm, long pcm_stride,
                     int *run_samples, int *samples, hipStream_t q)
{
    if (nruns <= 0) return 0;
    hipLaunchKernelGGL(L.hs ? k_run_plan<1> : k_run_plan<0>, dim3((nruns + 63) / 64), dim3(64), 0, q, L.s, nruns, runtab, L.status, L.info,
                       granulepos, eos, gap, L.prevW, L.gp, L.sc, plan, samples, run_samples, run_last);
    if (last_err()) return -2;
    if (L.nsb > 0) {
        hipLaunchKernelGGL(L.hs ? k_overlap_runs<1> : k_overlap_runs<0>, dim3(L.nsb), dim3(256), 0, q, L.s, runtab, L.status,
                           L.info, plan, L.imdct, L.n1, L.win0, L.win1, L.tail, pcm, pcm_stride, L.ohalf);
        if (last_err()) return -2;
        hipLaunchKernelGGL(L.hs ? k_run_commit<1> : k_run_commit<0>, dim3(nruns), dim3(256), 0, q, L.s, nruns, runtab, run_last,
                           L.info, L.imdct, L.n1, L.tail, L.ohalf);
    }
    return last_err();
}

int vbmd_launch_unpack_rows(const vbmd_launch &L, int npieces, const int *rtab, int *rows, const uint8_t *data,
                            const long long *offsets, long long data_bytes, hipStream_t q)
{
    if (L.nsb <= 0) return 0;
    hipLaunchKernelGGL(k_range_rows, dim3((npieces + 63) / 64), dim3(64), 0, q, npieces, rtab, rows);
    if (last_err()) return -2;
    hipLaunchKernelGGL(k_unpack_rows, dim3((L.nsb + 63) / 64), dim3(64), 0, q, L.s, L.blob, L.nsb, rows, data, offsets,
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
    hipLaunchKernelGGL(L.hs ? k_overlap_runs<1> : k_overlap_runs<0>, dim3(L.nsb), dim3(256), 0, q, L.s, runtab, L.status,
                       L.info, plan, L.imdct, L.n1, L.win0, L.win1, L.tail, pcm, pcm_stride, L.ohalf);
    return last_err();
}
