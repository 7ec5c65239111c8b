// What the kernels that write Ogg pages share (k_mux_emit in ogg_mux.hip, k_cut_emit in ogg_cut.hip) and the vector
// copy of the kernels that move runs of bytes (k_sel_copy in ogg_select.hip, k_cut_emit): the table step of the CRC,
// the CRC of a run read as aligned dwords, the combination of the lanes' chunk codes, and the two copies.  Device code
// only; the arithmetic of the code itself is ogg_mux.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ogg_mux.h"

__device__ __forceinline__ uint32_t crc_byte(const uint32_t *T, uint32_t crc, uint32_t b)
{
    return (crc << 8) ^ T[((crc >> 24) ^ b) & 0xff];
}

// crc over the n bytes at src: single bytes up to a dword boundary, whole dwords, single bytes
__device__ __forceinline__ uint32_t crc_run(const uint32_t *T, uint32_t crc, const uint8_t *src, int n)
{
    int i = 0;
    for (; i < n && ((uintptr_t)(src + i) & 3); i++) crc = crc_byte(T, crc, src[i]);
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = *(const uint32_t *)(src + i);
        crc = crc_byte(T, crc, w & 0xff);
        crc = crc_byte(T, crc, (w >> 8) & 0xff);
        crc = crc_byte(T, crc, (w >> 16) & 0xff);
        crc = crc_byte(T, crc, w >> 24);
    }
    for (; i < n; i++) crc = crc_byte(T, crc, src[i]);
    return crc;
}

// The page's code from the codes of the lanes' chunks: a lane whose chunk is followed by `after` bytes of the page
// (has == false: the lane took no byte) multiplies by x^(8 * after); the xor over the wavefront, in every lane
__device__ __forceinline__ uint32_t crc_wave_combine(const OggMuxPow &pw, uint32_t crc, bool has, uint32_t after)
{
    crc = has ? oggmux_crc_shift(pw, crc, after) : 0u;
    for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
    return crc;
}

// n bytes src -> dst by the 64 lanes of a wavefront, src and dst not overlapping; stores at or beyond `room` bytes
// from dst are dropped (second line of defence: the host has checked the capacity against the bound)
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, int n, long long room, int lane)
{
    if (n > room) n = room > 0 ? (int)room : 0;
    const int lead = min(n, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    if (lane < lead) dst[lane] = src[lane];
    const int nd = (n - lead) >> 2;
    const uint8_t *s0 = src + lead;
    const int sh = (int)((uintptr_t)s0 & 3) * 8;
    const uint32_t *sa = (const uint32_t *)(s0 - ((uintptr_t)s0 & 3));
    uint32_t *da = (uint32_t *)(dst + lead);
    if (sh == 0) {
        for (int i = lane; i < nd; i += 64) da[i] = sa[i];
    } else {
        // the dword after the last one read still holds a byte of the source: it lies inside the source's allocation
        for (int i = lane; i < nd; i += 64) da[i] = (sa[i] >> sh) | (sa[i + 1] << (32 - sh));
    }
    const int done = lead + nd * 4;
    if (lane < n - done) dst[done + lane] = src[done + lane];
}

// 16 bytes from byte 16 * i + 4 * q + r of the aligned words at sa (q, r in 0..3, not both 0): words i and i + 1
__device__ __forceinline__ uint4 vec_fetch(const uint4 *sa, int i, int q, int r)
{
    const uint4 a = sa[i], b = sa[i + 1];
    const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t s[5];
#pragma unroll
    for (int j = 0; j < 5; j++) s[j] = q == 0 ? x[j] : q == 1 ? x[j + 1] : q == 2 ? x[j + 2] : x[j + 3];
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = (uint32_t)((((unsigned long long)s[j + 1] << 32) | s[j]) >> (8 * r));
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// n bytes src -> dst by NT threads, of which this is thread t (a block of 256, or the 64 lanes of a wavefront).
// 16-byte stores to the aligned middle of dst.  A source that is not aligned with it is read as aligned 16-byte words:
// the first may begin up to 15 bytes in front of src (still inside the buffer's allocation, whose base is aligned), and
// none reaches past src + n: the buffer may end with this run.
template <int NT> __device__ __forceinline__ void vec_copy(uint8_t *dst, const uint8_t *src, int n, int t)
{
    const int lead = min(n, (int)((16 - ((uintptr_t)dst & 15)) & 15));
    if (t < lead) dst[t] = src[t];
    int nd = (n - lead) >> 4;
    const uint8_t *s0 = src + lead;
    const int sh = (int)((uintptr_t)s0 & 15);
    const uint4 *sa = (const uint4 *)(s0 - sh);
    uint4 *da = (uint4 *)(dst + lead);
    if (sh) {
        // word i needs sa[i] and sa[i + 1]: both must end at or before src + n
        const int whole = (int)((src + n - (const uint8_t *)sa) >> 4);
        nd = max(0, min(nd, whole - 1));
    }
    const int q = sh >> 2, r = sh & 3;
    for (int i0 = t; i0 < nd; i0 += 4 * NT) {       // four loads in flight per thread, then their stores
        uint4 v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = i0 + j * NT;
            if (i < nd) v[j] = sh ? vec_fetch(sa, i, q, r) : sa[i];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = i0 + j * NT;
            if (i < nd) da[i] = v[j];
        }
    }
    for (int i = lead + nd * 16 + t; i < n; i += NT) dst[i] = src[i];
}
