// The index of demuxed streams on the device (rules and the chunked scan: decode_index.h), and its host twin.
//
//   k_index_head   one lane per packet: vbmd_head on the packet's first bytes -> status, and W into begin []
//   k_index_scan   one wavefront per stream, grid-stride over streams: chunks of 64 packets with the stream's state
//                  carried from chunk to chunk; the scans are __shfl_up ladders.  A stream with a granulepos below
//                  -1 on a valid packet (found by all 64 lanes striding over it) is walked by lane 0 instead.
// No LDS, no scratch, no block-wide barrier: the four wavefronts of a block work on four streams on their own.
#include <hip/hip_runtime.h>
#include <climits>
#include <string>
#include <vector>

#include "decode_index.h"
#include "decode_kernels.h"
#include "decode_setup.h"
#include "vbm_internal.h"
#include "vorbis_mi355x.h"

namespace {

constexpr int kHeadBlocks = 1 << 16;   // most blocks k_index_head is launched with
constexpr int kScanBlocks = 2048;      // ... k_index_scan (four streams per block at a time)

struct vbmi_wave {                     // the 64 lanes of vbmi_chunk: a wavefront, one value per lane
    static constexpr int NL = 1;
    static __device__ __forceinline__ int lane(int) { return threadIdx.x & 63; }
    static __device__ __forceinline__ void excl_max(const int (&v)[1], int (&out)[1])
    {
        const int l = lane(0);
        int x = v[0];
        for (int dist = 1; dist < 64; dist <<= 1) {
            const int y = __shfl_up(x, dist, 64);
            if (l >= dist) x = max(x, y);
        }
        const int below = __shfl_up(x, 1, 64);
        out[0] = l ? below : -1;
    }
    static __device__ __forceinline__ void incl_sum(const int (&v)[1], int (&out)[1])
    {
        const int l = lane(0);
        int x = v[0];
        for (int dist = 1; dist < 64; dist <<= 1) {
            const int y = __shfl_up(x, dist, 64);
            if (l >= dist) x += y;
        }
        out[0] = x;
    }
    template <class T> static __device__ __forceinline__ void gather(const T (&v)[1], const int (&idx)[1], T (&out)[1])
    {
        out[0] = __shfl(v[0], idx[0] < 0 ? 0 : idx[0], 64);
    }
    static __device__ __forceinline__ vbmi_state last(const vbmi_state (&a)[1])
    {
        vbmi_state r;
        r.lastW = __shfl(a[0].lastW, 63, 64);
        r.hasj = __shfl(a[0].hasj, 63, 64);
        r.sc = __shfl(a[0].sc, 63, 64);
        r.jgp = __shfl(a[0].jgp, 63, 64);
        r.jsc = __shfl(a[0].jsc, 63, 64);
        r.at = __shfl(a[0].at, 63, 64);
        return r;
    }
};

struct vbmi_host_lanes {               // the same on the CPU: 64 values per quantity, the scans as loops
    static constexpr int NL = 64;
    static int lane(int i) { return i; }
    static void excl_max(const int (&v)[64], int (&out)[64])
    {
        int m = -1;
        for (int i = 0; i < 64; i++) {
            out[i] = m;
            if (v[i] > m) m = v[i];
        }
    }
    static void incl_sum(const int (&v)[64], int (&out)[64])
    {
        int s = 0;
        for (int i = 0; i < 64; i++) out[i] = s += v[i];
    }
    template <class T> static void gather(const T (&v)[64], const int (&idx)[64], T (&out)[64])
    {
        for (int i = 0; i < 64; i++) out[i] = v[idx[i] < 0 ? 0 : idx[i]];
    }
    static vbmi_state last(const vbmi_state (&a)[64]) { return a[63]; }
};

// MX: packets [k0, P) are those of the n streams of first [n + 1], whose classes [n] lie behind it; a lane finds its
// packet's stream by a search in first (vbmi_stream_of), hence its class's setup in the table
template <bool MX>
__global__ void __launch_bounds__(256) k_index_head(const vbmd_setup *s, const vbmd_class *table, const int *first,
                                                    int n, long long k0, long long P, const uint8_t *data,
                                                    const long long *offsets, long long data_bytes, int *status,
                                                    int *begin)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long k = k0 + (long long)blockIdx.x * 256 + threadIdx.x; k < P; k += stride) {
        int W;
        if (MX) s = table[first[n + 1 + vbmi_stream_of(first, n, k)]].s;
        status[k] = vbmi_head(*s, data, offsets, data_bytes, k, W);
        begin[k] = W;
    }
}

// MX: stream i takes its block sizes from the class first[nstreams + 1 + i] of the table, so the four wavefronts of a
// block may scan four streams of four classes
template <int HS, bool MX>
__global__ void __launch_bounds__(256) k_index_scan(const vbmd_setup *s, const vbmd_class *table, int nstreams,
                                                    const int *first, const int *status,
                                                    const long long *granulepos, const uint8_t *eos, int *begin,
                                                    int *end, long long *out_start, long long *out_end,
                                                    long long *totals)
{
    const int lane = threadIdx.x & 63;
    const int *bs = MX ? nullptr : s->blocksizes;
    const int nwaves = gridDim.x * 4;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nstreams; i += nwaves) {      // uniform over the wavefront
        if (MX) bs = table[first[nstreams + 1 + i]].s->blocksizes;
        const long long a = first[i], n = first[i + 1] - a;
        const long long *gp = granulepos ? granulepos + a : nullptr;
        const uint8_t *eo = eos ? eos + a : nullptr;
        long long *oe = out_end ? out_end + a : nullptr;
        int below = 0;
        if (gp)
            for (long long k = lane; k < n; k += 64) below |= status[a + k] == 0 && gp[k] < -1;
        if (__ballot(below) != 0) {
            if (lane == 0) vbmi_serial<HS>(bs, n, status + a, gp, eo, begin + a, end + a, out_start + a, oe, totals + i);
            continue;
        }
        vbmi_state st = vbmi_fresh();
        for (long long k0 = 0; k0 < n; k0 += 64)
            vbmi_chunk<vbmi_wave, HS>(bs, n - k0, status + a + k0, gp ? gp + k0 : nullptr, eo ? eo + k0 : nullptr,
                                      begin + a + k0, end + a + k0, out_start + a + k0, oe ? oe + k0 : nullptr, st);
        if (lane == 0) totals[i] = st.at;
    }
}

template <int HS>
void host_scan_stream(const int *bs, long long n, const int *status, const long long *gp, const uint8_t *eo, int *begin,
                      int *end, long long *out_start, long long *total)
{
    bool below = false;
    for (long long k = 0; gp && k < n; k++) below |= status[k] == 0 && gp[k] < -1;
    if (below) {
        vbmi_serial<HS>(bs, n, status, gp, eo, begin, end, out_start, nullptr, total);
        return;
    }
    vbmi_state st = vbmi_fresh();
    for (long long k0 = 0; k0 < n; k0 += 64)
        vbmi_chunk<vbmi_host_lanes, HS>(bs, n - k0, status + k0, gp ? gp + k0 : nullptr, eo ? eo + k0 : nullptr,
                                        begin + k0, end + k0, out_start + k0, nullptr, st);
    *total = st.at;
}

}  // namespace

int vbmd_launch_index_head(const vbmd_setup *d_setup, long long P, const uint8_t *d_data, const long long *d_offsets,
                           long long data_bytes, int *d_status, int *d_begin, hipStream_t q)
{
    if (P <= 0) return 0;
    const long long blocks = (P + 255) / 256;
    hipLaunchKernelGGL(k_index_head<false>, dim3((unsigned)(blocks < kHeadBlocks ? blocks : kHeadBlocks)), dim3(256), 0,
                       q, d_setup, nullptr, nullptr, 0, 0, P, d_data, d_offsets, data_bytes, d_status, d_begin);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int vbmd_launch_index_head_mixed(const vbmd_class *table, int nstreams, const int *d_first, long long k0, long long k1,
                                 const uint8_t *d_data, const long long *d_offsets, long long data_bytes, int *d_status,
                                 int *d_begin, hipStream_t q)
{
    if (k1 <= k0 || nstreams <= 0) return 0;
    const long long blocks = (k1 - k0 + 255) / 256;
    hipLaunchKernelGGL(k_index_head<true>, dim3((unsigned)(blocks < kHeadBlocks ? blocks : kHeadBlocks)), dim3(256), 0,
                       q, nullptr, table, d_first, nstreams, k0, k1, d_data, d_offsets, data_bytes, d_status, d_begin);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int vbmd_launch_index_scan(const vbmd_setup *d_setup, const vbmd_class *table, int halfrate, int nstreams,
                           const int *d_first, const int *d_status, const long long *d_granulepos, const uint8_t *d_eos, int *d_begin,
                           int *d_end, long long *d_out_start, long long *d_out_end, long long *d_totals, hipStream_t q)
{
    if (nstreams <= 0) return 0;
    const int blocks = (nstreams + 3) / 4;
    const dim3 grid((unsigned)(blocks < kScanBlocks ? blocks : kScanBlocks));
    const auto kernel = halfrate ? (table ? k_index_scan<1, true> : k_index_scan<1, false>)
                                 : (table ? k_index_scan<0, true> : k_index_scan<0, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, q, d_setup, table, nstreams, d_first, d_status, d_granulepos, d_eos,
                       d_begin, d_end, d_out_start, d_out_end, d_totals);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// the host twin over the streams of nclasses setups; classes null: every stream is of setups[0]
static int host_index_scan(int nclasses, const vbm_decode_setup *const *setups, int halfrate, int nstreams,
                           const long long *stream_packets, const int *classes, const uint8_t *data,
                           const long long *offsets, long long data_bytes, const long long *granulepos,
                           const uint8_t *eos, int *status, int *begin, int *end, long long *out_start,
                           long long *totals)
{
    if (halfrate != 0 && halfrate != 1) { g_vbm_err = "halfrate must be 0 or 1"; return VBM_EINVAL; }
    if (nclasses <= 0 || !setups || nstreams <= 0 || !stream_packets || data_bytes < 0 || (data_bytes > 0 && !data) ||
        !offsets || !totals)
        return VBM_EINVAL;
    if (stream_packets[0] != 0) { g_vbm_err = "stream_packets[0] must be 0"; return VBM_EINVAL; }
    for (int i = 0; i < nstreams; i++)
        if (stream_packets[i + 1] < stream_packets[i]) { g_vbm_err = "stream_packets must not decrease"; return VBM_EINVAL; }
    const long long P = stream_packets[nstreams];
    if (P >= INT_MAX) { g_vbm_err = "more than 2^31 - 2 packets in one index"; return VBM_EINVAL; }
    if (P > 0 && (!status || !begin || !end || !out_start)) return VBM_EINVAL;
    for (int c = 0; c < nclasses; c++)
        if (!setups[c]) return VBM_EINVAL;
    for (int i = 0; classes && i < nstreams; i++)
        if (classes[i] < 0 || classes[i] >= nclasses) {
            g_vbm_err = "stream " + std::to_string(i) + ": class id " + std::to_string(classes[i]) + " is not in the table";
            return VBM_EINVAL;
        }
    // the kernels' lookup: a packet's stream by vbmi_stream_of in the int table of first packets, then its class
    std::vector<int> first(stream_packets, stream_packets + nstreams + 1);
    for (long long k = 0; k < P; k++) {
        const vbm_decode_setup *ds = setups[classes ? classes[vbmi_stream_of(first.data(), nstreams, k)] : 0];
        status[k] = vbmi_head(ds->s, data, offsets, data_bytes, k, begin[k]);
    }
    for (int i = 0; i < nstreams; i++) {
        const long long a = stream_packets[i], n = stream_packets[i + 1] - a;
        const long long *gp = granulepos ? granulepos + a : nullptr;
        const uint8_t *eo = eos ? eos + a : nullptr;
        const int *bs = setups[classes ? classes[i] : 0]->s.blocksizes;
        if (halfrate) host_scan_stream<1>(bs, n, status + a, gp, eo, begin + a, end + a, out_start + a, totals + i);
        else host_scan_stream<0>(bs, n, status + a, gp, eo, begin + a, end + a, out_start + a, totals + i);
    }
    return VBM_OK;
}

extern "C" int vbm_host_decode_index_scan(const vbm_decode_setup *ds, int halfrate, int nstreams,
                                          const long long *stream_packets, const uint8_t *data,
                                          const long long *offsets, long long data_bytes, const long long *granulepos,
                                          const uint8_t *eos, int *status, int *begin, int *end, long long *out_start,
                                          long long *totals)
{
    if (!ds) {
        if (halfrate != 0 && halfrate != 1) g_vbm_err = "halfrate must be 0 or 1";
        return VBM_EINVAL;
    }
    return host_index_scan(1, &ds, halfrate, nstreams, stream_packets, nullptr, data, offsets, data_bytes, granulepos,
                           eos, status, begin, end, out_start, totals);
}

extern "C" int vbm_host_decode_index_scan_mixed(int nclasses, const vbm_decode_setup *const *setups, int halfrate,
                                                int nstreams, const long long *stream_packets,
                                                const int *stream_classes, const uint8_t *data,
                                                const long long *offsets, long long data_bytes,
                                                const long long *granulepos, const uint8_t *eos, int *status,
                                                int *begin, int *end, long long *out_start, long long *totals)
{
    if (halfrate != 0 && halfrate != 1) { g_vbm_err = "halfrate must be 0 or 1"; return VBM_EINVAL; }
    if (!stream_classes) return VBM_EINVAL;
    return host_index_scan(nclasses, setups, halfrate, nstreams, stream_packets, stream_classes, data, offsets,
                           data_bytes, granulepos, eos, status, begin, end, out_start, totals);
}
