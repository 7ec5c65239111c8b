// The kernels of the live range store (rules, layout and the order of an append: live_store.h).
//
//   k_live_plan     one lane per entry: vbml_plan_entry; a slot that trims and keeps packets goes onto the trimmed list
//                   (one atomic per entry on a counter the call has cleared)
//   k_live_compact  a fixed grid of workgroups of 256 that deals the trimmed list out: what a slot retains moves to the
//                   front of its region.  Source and destination overlap (dst < src), so a workgroup walks forward
//                   chunk by chunk: every thread loads its part of the chunk, a barrier, every thread stores it.  The
//                   stores of a chunk end below the first source byte of the next chunk, so one barrier per chunk is
//                   enough: a later chunk's loads never meet an earlier chunk's stores.  Bytes move as 16-byte words to
//                   the region's aligned front (a source that is not aligned with it as two aligned loads and a shift,
//                   vec_fetch), the ragged end as single bytes; the index entries 256 at a time.  A call in which no
//                   slot trims finds the list empty: every workgroup reads one int and leaves.
//   k_live_walk     one lane per entry, serial over its run (tens of packets; the parallelism is the entries, as in
//                   k_run_plan): vbml_walk_entry
//   k_live_copy     one workgroup of 256 per entry: its bytes are one run of the caller's CSR, which starts and lands
//                   at any residue mod 16 (vec_copy of ogg_emit.h: 16-byte stores to the aligned middle, single bytes at
//                   the ends)
// No LDS in any of them; every store is a plain vector store.
#include <hip/hip_runtime.h>

#include "decode_kernels.h"
#include "live_store.h"
#include "ogg_emit.h"

namespace {

constexpr int kCompactBlocks = 2048;   // k_live_compact's grid at most: eight workgroups per compute unit of 256

__global__ void __launch_bounds__(64) k_live_plan(vbml_arrays A, int n, const int *__restrict__ tab, int ids_at,
                                                  const long long *__restrict__ src_off, long long src_bytes,
                                                  vbml_plan *__restrict__ plans, int *__restrict__ trimmed)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    vbml_plan p;
    vbml_plan_entry(A, tab[ids_at + e], tab[e], tab[e + 1], src_off, src_bytes, p);
    plans[e] = p;
    if (p.drop > 0 && p.keep > 0) trimmed[1 + atomicAdd(trimmed, 1)] = e;
}

__global__ void __launch_bounds__(256) k_live_compact(vbml_arrays A, const vbml_plan *__restrict__ plans,
                                                      const int *__restrict__ trimmed)
{
    const int t = threadIdx.x, count = trimmed[0];
    for (int i = blockIdx.x; i < count; i += gridDim.x) {          // uniform over the workgroup
        const vbml_plan p = plans[trimmed[1 + i]];
        const long long P0 = (long long)p.sid * (A.MP + 1);
        // the index entries: packet drop + k -> k, and the keep + 1 offsets, which also lose the bytes cut off
        for (int k0 = 0; k0 <= p.keep; k0 += 256) {
            const int k = k0 + t;
            const long long from = P0 + p.drop + k, to = P0 + k;
            long long off = 0, os = 0;
            int st = 0, b = 0, e = 0;
            if (k <= p.keep) off = A.offsets[from] - p.cut;
            if (k < p.keep) {
                os = A.out_start[from];
                st = A.status[from];
                b = A.begin[from];
                e = A.end[from];
            }
            __syncthreads();
            if (k <= p.keep) A.offsets[to] = off;
            if (k < p.keep) {
                A.out_start[to] = os;
                A.status[to] = st;
                A.begin[to] = b;
                A.end[to] = e;
            }
        }
        // the bytes: [base + cut, base + cut + kept) -> base, which is 16-byte aligned
        uint8_t *dst = A.data + (long long)p.sid * A.stride;
        const uint8_t *src = dst + p.cut;
        const int sh = (int)((uintptr_t)src & 15), q = sh >> 2, r = sh & 3;
        const uint4 *sa = (const uint4 *)(src - sh);
        uint4 *da = (uint4 *)dst;
        long long nd = p.kept >> 4;
        if (sh) {                                                  // word w needs sa[w] and sa[w + 1], both inside the run
            const long long whole = (p.kept + sh) >> 4;
            nd = nd < whole - 1 ? nd : whole - 1;
            if (nd < 0) nd = 0;
        }
        for (long long w0 = 0; w0 < nd; w0 += 256) {
            const long long w = w0 + t;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (w < nd) v = sh ? vec_fetch(sa, (int)w, q, r) : sa[w];
            __syncthreads();
            if (w < nd) da[w] = v;
        }
        const long long done = nd * 16;                            // at most 31 bytes are left
        uint8_t last = 0;
        if (done + t < p.kept) last = src[done + t];
        __syncthreads();
        if (done + t < p.kept) dst[done + t] = last;
    }
}

template <int HS, bool MX>
__global__ void __launch_bounds__(64) k_live_walk(vbml_arrays A, const vbmd_setup *__restrict__ s,
                                                  const vbmd_class *__restrict__ table, int n,
                                                  const vbml_plan *__restrict__ plans,
                                                  const long long *__restrict__ src_off,
                                                  const int *__restrict__ head_status, const int *__restrict__ head_W,
                                                  const long long *__restrict__ granulepos,
                                                  const uint8_t *__restrict__ eos, const uint8_t *__restrict__ gap,
                                                  int *__restrict__ pk_status, long long *__restrict__ pk_out_end,
                                                  vbml_back *__restrict__ back)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const vbml_plan p = plans[e];
    if (MX) s = table[A.slots[p.sid].cls].s;
    vbml_back b;
    vbml_walk_entry<HS>(A, s->blocksizes, p, src_off, head_status, head_W, granulepos, eos, gap, pk_status, pk_out_end,
                        b);
    back[e] = b;
}

__global__ void __launch_bounds__(256) k_live_copy(vbml_arrays A, const vbml_plan *__restrict__ plans,
                                                   const uint8_t *__restrict__ src,
                                                   const long long *__restrict__ src_off)
{
    const vbml_plan p = plans[blockIdx.x];
    if (p.status) return;
    const long long a = src_off[p.k0], nb = src_off[p.k1] - a;      // 0 <= nb <= MB < 2^31: vbml_plan_entry
    uint8_t *dst = A.data + (long long)p.sid * A.stride + p.kept;   // kept + nb <= MB: vbml_drop
    vec_copy<256>(dst, src + a, (int)nb, threadIdx.x);
}

__global__ void k_live_restart(vbml_arrays A, int n, const int *__restrict__ ids, const int *__restrict__ cls)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int sid = ids[k];
    A.slots[sid] = vbml_fresh(cls ? cls[k] : A.slots[sid].cls);
}

inline int last_err() { return hipGetLastError() == hipSuccess ? 0 : -2; }

}  // namespace

int vbml_launch_append(const vbml_arrays &A, int halfrate, const vbmd_setup *bs_setup, const vbmd_class *table, int n,
                       const int *d_tab, int ids_at, const uint8_t *d_src, const long long *d_src_off,
                       long long src_bytes, const int *d_head_status, const int *d_head_W,
                       const long long *d_granulepos, const uint8_t *d_eos, const uint8_t *d_gap, vbml_plan *d_plans,
                       int *d_trimmed, int *d_pk_status, long long *d_pk_out_end, vbml_back *d_back, hipStream_t q)
{
    if (n <= 0) return 0;
    if (hipMemsetAsync(d_trimmed, 0, sizeof(int), q) != hipSuccess) return -2;
    const dim3 lanes((n + 63) / 64);
    hipLaunchKernelGGL(k_live_plan, lanes, dim3(64), 0, q, A, n, d_tab, ids_at, d_src_off, src_bytes, d_plans, d_trimmed);
    if (last_err()) return -2;
    hipLaunchKernelGGL(k_live_compact, dim3(n < kCompactBlocks ? n : kCompactBlocks), dim3(256), 0, q, A, d_plans,
                       d_trimmed);
    if (last_err()) return -2;
    const auto walk = halfrate ? (table ? k_live_walk<1, true> : k_live_walk<1, false>)
                               : (table ? k_live_walk<0, true> : k_live_walk<0, false>);
    hipLaunchKernelGGL(walk, lanes, dim3(64), 0, q, A, bs_setup, table, n, d_plans, d_src_off, d_head_status, d_head_W,
                       d_granulepos, d_eos, d_gap, d_pk_status, d_pk_out_end, d_back);
    if (last_err()) return -2;
    hipLaunchKernelGGL(k_live_copy, dim3(n), dim3(256), 0, q, A, d_plans, d_src, d_src_off);
    return last_err();
}

int vbml_launch_restart(const vbml_arrays &A, int n, const int *d_ids, const int *d_cls, hipStream_t q)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_live_restart, dim3((n + 255) / 256), dim3(256), 0, q, A, n, d_ids, d_cls);
    return last_err();
}
