// Butterflies and bit-reverse of the reference's MDCT (lib/mdct.c:432-658 mdct_butterfly_*, :1105-1135
// mdct_butterflies, :1228-1272 mdct_bitreverse), wavefront-wide on 512-complex groups.  Shared by the forward kernels
// (mdct_kernel.hip: mdct_forward) and the backward kernels (decode_kernels.hip: mdct_backward), which call the same two
// routines (lib/mdct.c:1276-1537 scalar branch).  Every butterfly keeps the source expression shape; compile with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace vbm_mdct {

constexpr float K_PI3_8 = .38268343236508977175F;  // lib/mdct.h:44-46
constexpr float K_PI2_8 = .70710678118654752441F;
constexpr float K_PI1_8 = .92387953251128675613F;

constexpr int SLOTS = 576;  // 512 complex + 1 pad slot per 8 (bank-conflict-free transposes)

__device__ __forceinline__ int slot_addr(int m) { return m + (m >> 3); }

// wave-level ordering of LDS traffic: DS ops of one wave execute in issue order, so all
// that is needed is that the compiler neither reorders nor caches across this point.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// lo' = rot(up - lo), up' = up + lo      (lib/mdct.c:1044-1049 expression shape)
__device__ __forceinline__ void bfly(float2 &lo, float2 &up, float2 w)
{
    float r0 = up.x - lo.x;
    float r1 = up.y - lo.y;
    up.x += lo.x;
    up.y += lo.y;
    lo.x = r1 * w.y + r0 * w.x;
    lo.y = r1 * w.x - r0 * w.y;
}

// lib/mdct.c:432-452
__device__ __forceinline__ void bfly8(float *x)
{
    float a = x[6] + x[2], b = x[6] - x[2];
    float c = x[4] + x[0], d = x[4] - x[0];
    float e = x[5] - x[1], f = x[7] - x[3];
    float g = x[5] + x[1], h = x[7] + x[3];
    x[6] = a + c;
    x[4] = a - c;
    x[0] = b + e;
    x[2] = b - e;
    x[3] = f + d;
    x[1] = f - d;
    x[7] = h + g;
    x[5] = h - g;
}

// lib/mdct.c:495-528
__device__ __forceinline__ void bfly16(float *x)
{
    float r0, r1;
    r0 = x[1] - x[9];   r1 = x[0] - x[8];
    x[8] += x[0];   x[9] += x[1];
    x[0] = (r0 + r1) * K_PI2_8;
    x[1] = (r0 - r1) * K_PI2_8;
    r0 = x[3] - x[11];  r1 = x[10] - x[2];
    x[10] += x[2];  x[11] += x[3];
    x[2] = r0;  x[3] = r1;
    r0 = x[12] - x[4];  r1 = x[13] - x[5];
    x[12] += x[4];  x[13] += x[5];
    x[4] = (r0 - r1) * K_PI2_8;
    x[5] = (r0 + r1) * K_PI2_8;
    r0 = x[14] - x[6];  r1 = x[15] - x[7];
    x[14] += x[6];  x[15] += x[7];
    x[6] = r0;  x[7] = r1;
    bfly8(x);
    bfly8(x + 8);
}

// Radix rounds A, B, C on one 512-complex group held as c[k] = element lane + 64k: the butterfly stages of
// mdct_butterflies (lib/mdct.c:1105-1135) for index bits 8..4 — those the block size has — and the 32-point
// butterflies; the result is left in sx in natural order (slot 8*lane + k at padded address 9*lane + k).
// LOG2C = log2 of the complex length of the transform the group belongs to (9: a 2048 block = the group;
// 10: one half of a 4096 block after its first stage; 8, 7, 6, 5: two, four, eight, sixteen blocks per group).
template <int LOG2C>
__device__ __forceinline__ void radix_rounds(float2 (&c)[8], float2 *sx, const float *s_trig, const int lane)
{
        // ---------------- round A: index bits 8,7,6 of the blocks that have them ----------
        // trigint of the stage pairing index bit b is 4 << (LOG2C - 1 - b): the first butterfly of a block
        // steps the table by 4, every later stage doubles it (lib/mdct.c:1105-1135)
        if (LOG2C >= 9) {
            constexpr int TI = 4 << (LOG2C >= 9 ? LOG2C - 9 : 0);
#pragma unroll
            for (int k = 0; k < 4; k++) {  // bit 8
                int t = 255 - (lane + 64 * k);
                bfly(c[k], c[k + 4], *reinterpret_cast<const float2 *>(s_trig + TI * t));
            }
        }
        if (LOG2C >= 8) {
            constexpr int TI = 4 << (LOG2C >= 8 ? LOG2C - 8 : 0);
#pragma unroll
            for (int kb = 0; kb < 8; kb += 4)
#pragma unroll
                for (int k = 0; k < 2; k++) {  // bit 7
                    int t = 127 - (lane + 64 * k);
                    bfly(c[kb + k], c[kb + k + 2], *reinterpret_cast<const float2 *>(s_trig + TI * t));
                }
        }
        if (LOG2C >= 7) {
            constexpr int TI = 4 << (LOG2C >= 7 ? LOG2C - 7 : 0);
            int t = 63 - lane;  // bit 6
            float2 w = *reinterpret_cast<const float2 *>(s_trig + TI * t);
#pragma unroll
            for (int kb = 0; kb < 8; kb += 2) bfly(c[kb], c[kb + 1], w);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) sx[slot_addr(lane + 64 * k)] = c[k];
        wave_lds_sync();

        // ---------------- round B: index bits 5,4 ------------------------------------
        {
            const int base = (lane >> 3) * 64 + (lane & 7);
#pragma unroll
            for (int k = 0; k < 8; k++) c[k] = sx[slot_addr(base + 8 * k)];
            constexpr int MUL0 = (LOG2C >= 6) ? (4 << (LOG2C >= 6 ? LOG2C - 6 : 0)) : 0;  // trigint of the 64-complex stage
            constexpr int MUL1 = 4 << (LOG2C - 5);  // trigint of the 32-complex stage
            if (LOG2C >= 6) {   // 128-point blocks (32 complex) have no 64-complex stage
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    int t = 31 - ((lane & 7) + 8 * k);
                    bfly(c[k], c[k + 4], *reinterpret_cast<const float2 *>(s_trig + MUL0 * t));
                }
            }
#pragma unroll
            for (int kb = 0; kb < 8; kb += 4)
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    int t = 15 - ((lane & 7) + 8 * k);
                    bfly(c[kb + k], c[kb + k + 2], *reinterpret_cast<const float2 *>(s_trig + MUL1 * t));
                }
            wave_lds_sync();
#pragma unroll
            for (int k = 0; k < 8; k++) sx[slot_addr(base + 8 * k)] = c[k];
        }
        wave_lds_sync();

        // ---------------- round C: 32-point butterflies (lib/mdct.c:602-658) ----------
        float x[16];
        {
            // slots 8*lane .. 8*lane+7 are contiguous at padded address 9*lane (8-B units);
            // 9*lane*8 bytes is only 8-B aligned, so read as float2
#pragma unroll
            for (int k = 0; k < 8; k++) {
                float2 t = sx[9 * lane + k];
                x[2 * k] = t.x;
                x[2 * k + 1] = t.y;
            }
        }
        {
            float y[16];
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = __shfl_xor(x[j], 1);
            if (lane & 1) {
                // upper half of the 32-block: x[16+j] += x[j]
#pragma unroll
                for (int j = 0; j < 16; j++) x[j] = x[j] + y[j];
            } else {
                // lower half: differences (upper - lower, or as the source has it) rotated
                float r0, r1;
                r0 = x[0] - y[0];   r1 = x[1] - y[1];
                x[0] = r1 * K_PI3_8 + r0 * K_PI1_8;
                x[1] = r1 * K_PI1_8 - r0 * K_PI3_8;
                r0 = x[2] - y[2];   r1 = x[3] - y[3];
                x[2] = (r1 + r0) * K_PI2_8;
                x[3] = (r1 - r0) * K_PI2_8;
                r0 = x[4] - y[4];   r1 = x[5] - y[5];
                x[4] = r1 * K_PI1_8 + r0 * K_PI3_8;
                x[5] = r1 * K_PI3_8 - r0 * K_PI1_8;
                r0 = y[6] - x[6];   r1 = x[7] - y[7];
                x[6] = r1;  x[7] = r0;
                r0 = y[8] - x[8];   r1 = y[9] - x[9];
                x[8] = r0 * K_PI3_8 - r1 * K_PI1_8;
                x[9] = r1 * K_PI3_8 + r0 * K_PI1_8;
                r0 = y[10] - x[10]; r1 = y[11] - x[11];
                x[10] = (r0 - r1) * K_PI2_8;
                x[11] = (r0 + r1) * K_PI2_8;
                r0 = y[12] - x[12]; r1 = y[13] - x[13];
                x[12] = r0 * K_PI1_8 - r1 * K_PI3_8;
                x[13] = r0 * K_PI3_8 + r1 * K_PI1_8;
                r0 = y[14] - x[14]; r1 = y[15] - x[15];
                x[14] = r0;  x[15] = r1;
            }
        }
        bfly16(x);
        wave_lds_sync();
#pragma unroll
        for (int k = 0; k < 8; k++) sx[9 * lane + k] = make_float2(x[2 * k], x[2 * k + 1]);
        wave_lds_sync();

}

// one step of mdct_bitreverse: the complex values X0, X1 at the bit-reversed slots of pair u and the twiddle
// T = trig[n + 2u] -> w0 pair u (wA) and w1 pair C-1-u (wB).  A macro, not a function: the forward kernels keep the
// instruction selection they had when this was written out in each of them.
#define VBM_MDCT_BITREV_PAIR(X0, X1, T, wA, wB)                  \
    do {                                                         \
        float r0_ = (X0).y - (X1).y;                             \
        float r1_ = (X0).x + (X1).x;                             \
        float r2_ = r1_ * (T).x + r0_ * (T).y;                   \
        float r3_ = r1_ * (T).y - r0_ * (T).x;                   \
        float h0_ = ((X0).y + (X1).y) * .5f;                     \
        float h1_ = ((X0).x - (X1).x) * .5f;                     \
        wA = make_float2(h0_ + r2_, h1_ + r3_);                  \
        wB = make_float2(h0_ - r2_, r3_ - h1_);                  \
    } while (0)

// slots read by pair u of a 2^LOG2C-complex transform: bitrev[2u] / 2 = s0, bitrev[2u+1] / 2 = s1
#define VBM_MDCT_BITREV_SLOTS(LOG2C, C, u, s0, s1)                          \
    do {                                                                    \
        const int rv_ = (int)(__brev((unsigned)(u)) >> (32 - ((LOG2C) - 1))); \
        s1 = 2 * rv_;                                                       \
        s0 = ((C) - 1) - 2 * rv_;                                           \
    } while (0)

}  // namespace vbm_mdct
