// Ogg paging on the device for every stream of a call at once (rule and sizes: ogg_mux.h), its host twin, and the
// C ABI over both (include/vorbis_mi355x.h, "stream wrapper, device form"; host scaffold: twin_host.h).
//
//   k_mux_index   one lane per row: the row joins its stream's list (order of the appends is free: plan sorts)
//   k_mux_plan    one lane per stream: sort by packetno, queue the lacing values, run the rule, record the pages
//   k_mux_scan    one block: exclusive scan of the streams' output bytes -> d_offsets
//   k_mux_emit    one wavefront per stream with a page to write or a queue to keep: header, lacing table and body
//                 written by all lanes (dword stores; misaligned sources through two aligned loads and a funnel
//                 shift), CRC in 64 contiguous chunks combined by the linearity of the code, then the commit: what
//                 the pages did not take becomes the queue of the next call
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string.h>
#include <new>
#include <string>
#include <vector>

#include "ogg_emit.h"
#include "ogg_mux.h"
#include "twin_host.h"

#define OGGMUX_MAX_ROWS 64   // rows per stream per call the emit kernel's piece table holds

namespace {

// ---- kernels ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_mux_index(int nrows, const vbm_packet_info *info, const int *packet_bytes,
                                                   int nstreams, int max_rows, int *count, int *rows, int *status)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nrows || packet_bytes[k] < 0) return;
    const int s = info[k].stream;
    if (s < 0) return;
    if (s >= nstreams) {
        atomicAdd(&status[nstreams], 1);
        return;
    }
    const int slot = atomicAdd(&count[s], 1);
    if (slot < max_rows) rows[(size_t)s * max_rows + slot] = k;
}

__global__ void __launch_bounds__(64) k_mux_plan(OggMuxDims d, OggMuxHead *head, uint8_t *lacing, long long *gran,
                                                 int *rows, int *count, const int *packet_bytes,
                                                 const vbm_packet_info *info, int flush, OggMuxPage *pages,
                                                 OggMuxCall *call, long long *sizes, int *status)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= d.nstreams) return;
    const int cnt = count[s];
    count[s] = 0;                                   // ready for the next call's index
    OggMuxHead h = head[s];
    OggMuxCall c;
    status[s] = oggmux_plan_stream(d, h, lacing + (size_t)s * d.lace_cap, gran + (size_t)s * d.lace_cap,
                                   rows + (size_t)s * d.max_rows, cnt, packet_bytes, info, flush,
                                   pages + (size_t)s * d.max_pages, c);
    c.pad[0] = c.pad[1] = c.pad[2] = 0;
    call[s] = c;
    sizes[s] = c.out_bytes;                         // compact for the scan: one block reads them all
    head[s].pageno = h.pageno;                      // nseg / nbody: commit
    head[s].flags = h.flags;
}

// 16 consecutive values per lane, loaded before any is used (one lane's 128 bytes are one cache line)
__global__ void __launch_bounds__(1024) k_mux_scan(int nstreams, const long long *sizes, long long *offsets)
{
    __shared__ long long wave_sum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long carry = 0;
    for (int base = 0; base < nstreams; base += 16 * 1024) {
        const int lo = base + t * 16;
        long long v[16], sum = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = lo + j < nstreams ? sizes[lo + j] : 0;
#pragma unroll
        for (int j = 0; j < 16; j++) sum += v[j];
        long long x = sum;                          // inclusive scan inside the wavefront
        for (int dist = 1; dist < 64; dist <<= 1) {
            const long long y = __shfl_up(x, dist, 64);
            if (lane >= dist) x += y;
        }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        long long at = carry + x - sum, total = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wave) at += wave_sum[w];
            total += wave_sum[w];
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (lo + j < nstreams) offsets[lo + j] = at;
            at += v[j];
        }
        carry += total;
        __syncthreads();                            // wave_sum is rewritten by the next tile
    }
    if (t == 0) offsets[nstreams] = carry;
}

__global__ void __launch_bounds__(64) k_mux_emit(OggMuxDims d, OggMuxPow pw, int qstride, OggMuxHead *head,
                                                 uint8_t *lacing, long long *gran, uint8_t *body, const int *rows,
                                                 const OggMuxPage *pages, const OggMuxCall *call,
                                                 const uint8_t *packets, long long packet_stride,
                                                 const int *packet_bytes, const long long *offsets, uint8_t *out,
                                                 long long out_capacity)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const OggMuxCall c = call[s];
    if (c.npages == 0 && c.nrows == 0) return;      // nothing written, queue as it was

    __shared__ uint32_t T[256];
    __shared__ uint8_t hdr[27 + 255 + 2];
    __shared__ int piece_off[OGGMUX_MAX_ROWS + 2];
    __shared__ const uint8_t *piece_ptr[OGGMUX_MAX_ROWS + 1];

    uint8_t *q = body + (size_t)s * qstride;
    uint8_t *lac = lacing + (size_t)s * d.lace_cap;
    long long *gr = gran + (size_t)s * d.lace_cap;
    for (int i = lane; i < 256; i += 64) T[i] = oggmux_crc_entry(i);
    const int np = c.nrows + 1;                     // pieces of the virtual body: the queue, then the packets taken
    if (lane == 0) {
        piece_off[0] = 0;
        piece_ptr[0] = q;
        int at = c.nbody_old;
        for (int j = 0; j < c.nrows; j++) {
            const int r = rows[(size_t)s * d.max_rows + j];
            piece_off[j + 1] = at;
            piece_ptr[j + 1] = packets + (size_t)r * packet_stride;
            at += packet_bytes[r];
        }
        piece_off[np] = at;
    }
    __syncthreads();

    const int serialno = head[s].serialno;
    long long at_out = offsets[s];
    for (int p = 0; p < c.npages; p++) {
        const OggMuxPage pg = pages[(size_t)s * d.max_pages + p];
        const int hl = 27 + pg.nseg, L = hl + pg.body_bytes;
        if (lane == 0) oggmux_page_header(pg, serialno, hdr);
        for (int i = lane; i < pg.nseg; i += 64) hdr[27 + i] = lac[pg.lace_at + i];
        __syncthreads();

        // CRC: lane l takes bytes [l * chunk, (l + 1) * chunk) of the page, then multiplies by x^(8 * bytes after it)
        const int chunk = (L + 63) >> 6;
        int a = lane * chunk, b = min(L, a + chunk);
        uint32_t crc = 0;
        if (a < b) {
            int pos = a;
            for (; pos < b && pos < hl; pos++) crc = crc_byte(T, crc, hdr[pos]);
            if (pos < b) {
                int v = pg.body_at + pos - hl;
                const int vend = pg.body_at + b - hl;
                int k = 0;
                while (piece_off[k + 1] <= v) k++;
                while (v < vend) {
                    const int pe = min(vend, piece_off[k + 1]);
                    const uint8_t *src = piece_ptr[k] + (v - piece_off[k]);
                    const int n = pe - v;
                    crc = crc_run(T, crc, src, n);
                    v = pe;
                    k++;
                }
            }
        }
        crc = crc_wave_combine(pw, crc, a < b, (uint32_t)(L - b));
        if (lane < 4) hdr[22 + lane] = (uint8_t)((crc >> (8 * lane)) & 0xff);
        __syncthreads();

        // write the page
        uint8_t *dst = out + at_out;
        long long room = out_capacity - at_out;
        for (int i = lane; i < hl; i += 64)
            if (i < room) dst[i] = hdr[i];
        dst += hl;
        room -= hl;
        int v = pg.body_at;
        const int vend = pg.body_at + pg.body_bytes;
        for (int k = 0; k < np && v < vend; k++) {
            if (piece_off[k + 1] <= v) continue;
            const int pe = min(vend, piece_off[k + 1]), n = pe - v;
            wave_copy(dst, piece_ptr[k] + (v - piece_off[k]), n, room, lane);
            dst += n;
            room -= n;
            v = pe;
        }
        at_out += L;
        __syncthreads();                            // hdr is rewritten for the next page
    }

    // ---- commit: virtual body [body_used, body_total) and lacing [lace_used, lace_total) become the queue ----------
    const int used = c.body_used;
    if (used > 0 && used < c.nbody_old) {
        // the rest of the old queue moves down in place: ascending 64-byte steps, each read whole before it is written
        const int n = c.nbody_old - used;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            uint8_t x = 0;
            if (i < n) x = q[used + i];
            __syncthreads();
            if (i < n) q[i] = x;
            __syncthreads();
        }
    }
    __syncthreads();
    for (int k = 1; k < np; k++) {
        const int lo = max(piece_off[k], used), hi = piece_off[k + 1];
        if (lo < hi) wave_copy(q + (lo - used), piece_ptr[k] + (lo - piece_off[k]), hi - lo, (long long)d.queue_bytes - (lo - used), lane);
    }
    const int keep = c.lace_total - c.lace_used;    // <= 254
    if (c.lace_used > 0 && keep > 0) {
        uint8_t lv[4];
        long long gv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = j * 64 + lane;
            lv[j] = i < keep ? lac[c.lace_used + i] : 0;
            gv[j] = i < keep ? gr[c.lace_used + i] : 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = j * 64 + lane;
            if (i < keep) {
                lac[i] = lv[j];
                gr[i] = gv[j];
            }
        }
    }
    if (lane == 0) {
        head[s].nseg = keep;
        head[s].nbody = c.body_total - used;
    }
}

__global__ void __launch_bounds__(256) k_mux_reset(int n, const int *start, OggMuxHead *head, int *count)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int s = start[3 * k];
    OggMuxHead h = {};
    h.serialno = start[3 * k + 1];
    h.pageno = start[3 * k + 2];
    h.flags = OGGMUX_STARTED;
    head[s] = h;
    count[s] = 0;
}

}  // namespace

// ---- host side (scaffold: twin_host.h) --------------------------------------------------------------------------

struct vbm_ogg_mux {
    OggMuxDims d;
    bool host = false;
    const vbm_setup_handle *setup = nullptr;
    OggMuxPow pow;
    int qstride = 0;
    TwinMem mem;                        // owns the per-stream state and the call scratch
    OggMuxHead *head = nullptr;
    uint8_t *lacing = nullptr;
    long long *gran = nullptr;
    uint8_t *body = nullptr;
    int *rows = nullptr, *count = nullptr;
    OggMuxPage *pages = nullptr;
    OggMuxCall *call = nullptr;
    long long *sizes = nullptr;         // device mux: out_bytes of every stream, compact
    int *d_start = nullptr;             // [3 * nstreams] stream, serialno, pageno of vbm_ogg_mux_start_streams
    std::vector<int> h_start;
};

namespace {

int create(vbm_ogg_mux **out, const vbm_setup_handle *setup, int nstreams, int max_packet_bytes, int max_rows,
           int queue_bytes, bool host)
{
    if (!out || !setup || nstreams < 1 || max_packet_bytes < 1 || max_packet_bytes > (1 << 24) || max_rows < 0 ||
        max_rows > OGGMUX_MAX_ROWS || queue_bytes < 0)
        return fail(VBM_EINVAL, "vbm_ogg_mux_create: bad argument (nstreams >= 1, 1 <= max_packet_bytes <= 2^24, "
                                "max_rows_per_stream <= 64, queue_bytes >= 0)");
    if (!host) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(VBM_ENODEV, "vbm_ogg_mux_create: no HIP device");
    }
    vbm_ogg_mux *m = new (std::nothrow) vbm_ogg_mux();
    if (!m) return fail(VBM_EFAULT, "vbm_ogg_mux_create: out of memory");
    m->host = m->mem.host = host;
    m->setup = setup;
    m->d = oggmux_dims(nstreams, max_packet_bytes, max_rows ? max_rows : 16, queue_bytes);
    m->pow = oggmux_pow_table();
    m->qstride = (m->d.queue_bytes + 15) & ~15;
    const size_t S = (size_t)nstreams;
    const char *who = "vbm_ogg_mux";
    int rc = m->mem.get(m->head, S, who);
    if (!rc) rc = m->mem.get(m->lacing, S * m->d.lace_cap, who);
    if (!rc) rc = m->mem.get(m->gran, S * m->d.lace_cap, who);
    if (!rc) rc = m->mem.get(m->body, S * m->qstride, who);
    if (!rc) rc = m->mem.get(m->rows, S * m->d.max_rows, who);
    if (!rc) rc = m->mem.get(m->count, S, who);
    if (!rc) rc = m->mem.get(m->pages, S * m->d.max_pages, who);
    if (!rc) rc = m->mem.get(m->call, S, who);
    if (!rc && !host) rc = m->mem.get(m->sizes, S, who);
    if (!rc && !host) rc = m->mem.get(m->d_start, S * 3, who);
    if (rc) {
        vbm_ogg_mux_destroy(m);
        return rc;
    }
    *out = m;
    return VBM_OK;
}

int check_call(const vbm_ogg_mux *m, bool host, const uint8_t *packets, long long packet_stride, const int *packet_bytes,
               const vbm_packet_info *info, int nrows, uint8_t *out, long long out_capacity, long long *offsets,
               int *status, const char *who)
{
    if (int rc = check_kind(m, host, who, "mux")) return rc;
    if (nrows < 0 || (nrows && (!packets || !packet_bytes || !info)) || !out || !offsets || !status)
        return fail(VBM_EINVAL, std::string(who) + ": null pointer or negative row count");
    if (nrows > 0 && packet_stride < m->d.max_packet_bytes)
        return fail(VBM_EINVAL, std::string(who) + ": packet_stride is smaller than max_packet_bytes");
    const long long need = oggmux_out_bound(m->d, nrows);
    if (out_capacity < need)
        return fail(VBM_EINVAL, std::string(who) + ": out_capacity " + std::to_string(out_capacity) + " is below vbm_ogg_mux_out_bound = " + std::to_string(need));
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_ogg_mux_create(vbm_ogg_mux **mux, const vbm_setup_handle *setup, int nstreams, int max_packet_bytes,
                                  int max_rows_per_stream, int queue_bytes)
{
    return create(mux, setup, nstreams, max_packet_bytes, max_rows_per_stream, queue_bytes, false);
}

extern "C" int vbm_host_ogg_mux_create(vbm_ogg_mux **mux, const vbm_setup_handle *setup, int nstreams,
                                       int max_packet_bytes, int max_rows_per_stream, int queue_bytes)
{
    return create(mux, setup, nstreams, max_packet_bytes, max_rows_per_stream, queue_bytes, true);
}

extern "C" void vbm_ogg_mux_destroy(vbm_ogg_mux *m)
{
    if (!m) return;
    m->mem.free_all();
    delete m;
}

extern "C" long long vbm_ogg_mux_out_bound(const vbm_ogg_mux *m, int nrows)
{
    if (!m || nrows < 0) return fail(VBM_EINVAL, "vbm_ogg_mux_out_bound: bad argument");
    return oggmux_out_bound(m->d, nrows);
}

extern "C" int vbm_ogg_mux_start_streams(vbm_ogg_mux *m, const int *stream_ids, int n, const int *serialnos,
                                         const char *vendor, const char *const *comments, int ncomments,
                                         uint8_t *host_buf, long long cap, long long *host_offsets, void *stream)
{
    if (!m || n < 0 || (n && (!stream_ids || !serialnos)) || !host_offsets || ncomments < 0 || (ncomments && !comments))
        return fail(VBM_EINVAL, "vbm_ogg_mux_start_streams: bad argument");
    for (int k = 0; k < n; k++) {
        if (stream_ids[k] < 0 || stream_ids[k] >= m->d.nstreams)
            return fail(VBM_EINVAL, "vbm_ogg_mux_start_streams: stream index out of range");
        for (int j = 0; j < k; j++)
            if (stream_ids[j] == stream_ids[k]) return fail(VBM_EINVAL, "vbm_ogg_mux_start_streams: a stream is listed twice");
    }
    // the three header packets are the same for every stream; only the serial number in the page headers differs
    long lens[3];
    int rc = vbm_header_packets(m->setup, vendor, comments, ncomments, nullptr, 0, lens);
    if (rc) return rc;
    std::vector<uint8_t> hp((size_t)(lens[0] + lens[1] + lens[2]));
    rc = vbm_header_packets(m->setup, vendor, comments, ncomments, hp.data(), (long)hp.size(), lens);
    if (rc) return rc;
    std::vector<uint8_t> all;
    std::vector<int> start;
    host_offsets[0] = 0;
    for (int k = 0; k < n; k++) {
        vbm_ogg_stream *os = nullptr;
        rc = vbm_ogg_stream_create(&os, serialnos[k]);
        if (rc) return rc;
        long at = 0;
        for (int i = 0; i < 3 && !rc; at += lens[i], i++) rc = vbm_ogg_stream_packetin(os, hp.data() + at, lens[i], 0, 0);
        int npages = 0;
        const uint8_t *page;
        long bytes;
        while (!rc && vbm_ogg_stream_pageout(os, 1, &page, &bytes) == 1) {
            all.insert(all.end(), page, page + bytes);
            npages++;
        }
        vbm_ogg_stream_destroy(os);
        if (rc) return rc;
        host_offsets[k + 1] = (long long)all.size();
        start.push_back(stream_ids[k]);
        start.push_back(serialnos[k]);
        start.push_back(npages);
    }
    if (!host_buf) return VBM_OK;   // size query: host_offsets[n] bytes
    if (cap < (long long)all.size()) return fail(VBM_EINVAL, "vbm_ogg_mux_start_streams: host_buf is too small");
    if (!all.empty()) memcpy(host_buf, all.data(), all.size());
    if (n == 0) return VBM_OK;
    if (m->host) {
        for (int k = 0; k < n; k++) {
            OggMuxHead h = {};
            h.serialno = start[3 * k + 1];
            h.pageno = start[3 * k + 2];
            h.flags = OGGMUX_STARTED;
            m->head[start[3 * k]] = h;
        }
        return VBM_OK;
    }
    hipStream_t q = (hipStream_t)stream;
    m->h_start = start;
    hipError_t e = hipMemcpyAsync(m->d_start, m->h_start.data(), sizeof(int) * 3 * n, hipMemcpyHostToDevice, q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_ogg_mux_start_streams: upload");
    hipLaunchKernelGGL(k_mux_reset, dim3((n + 255) / 256), dim3(256), 0, q, n, m->d_start, m->head, m->count);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(q);   // h_start / d_start are free for the next start
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_mux_start_streams");
}

extern "C" int vbm_ogg_mux_packets(vbm_ogg_mux *m, const uint8_t *d_packets, long long packet_stride,
                                   const int *d_packet_bytes, const vbm_packet_info *d_info, int nrows, int flush,
                                   uint8_t *d_out, long long out_capacity, long long *d_offsets, int *d_status,
                                   void *stream)
{
    int rc = check_call(m, false, d_packets, packet_stride, d_packet_bytes, d_info, nrows, d_out, out_capacity, d_offsets,
                        d_status, "vbm_ogg_mux_packets");
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    const OggMuxDims &d = m->d;
    hipError_t e = hipMemsetAsync(d_status + d.nstreams, 0, sizeof(int), q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_ogg_mux_packets: memset");
    if (nrows > 0)
        hipLaunchKernelGGL(k_mux_index, dim3((nrows + 255) / 256), dim3(256), 0, q, nrows, d_info, d_packet_bytes,
                           d.nstreams, d.max_rows, m->count, m->rows, d_status);
    hipLaunchKernelGGL(k_mux_plan, dim3((d.nstreams + 63) / 64), dim3(64), 0, q, d, m->head, m->lacing, m->gran, m->rows,
                       m->count, d_packet_bytes, d_info, flush ? 1 : 0, m->pages, m->call, m->sizes, d_status);
    hipLaunchKernelGGL(k_mux_scan, dim3(1), dim3(1024), 0, q, d.nstreams, m->sizes, d_offsets);
    hipLaunchKernelGGL(k_mux_emit, dim3(d.nstreams), dim3(64), 0, q, d, m->pow, m->qstride, m->head, m->lacing, m->gran,
                       m->body, m->rows, m->pages, m->call, d_packets, packet_stride, d_packet_bytes, d_offsets, d_out,
                       out_capacity);
    e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_mux_packets: launch");
}

// The same on the CPU: the rule of ogg_mux.h per stream, then a serial emit (table CRC) and commit.
extern "C" int vbm_host_ogg_mux_packets(vbm_ogg_mux *m, const uint8_t *packets, long long packet_stride,
                                        const int *packet_bytes, const vbm_packet_info *info, int nrows, int flush,
                                        uint8_t *out, long long out_capacity, long long *offsets, int *status)
{
    int rc = check_call(m, true, packets, packet_stride, packet_bytes, info, nrows, out, out_capacity, offsets, status,
                        "vbm_host_ogg_mux_packets");
    if (rc) return rc;
    const OggMuxDims &d = m->d;
    const CrcTable &T = crc_table();
    status[d.nstreams] = 0;
    for (int k = 0; k < nrows; k++) {
        if (packet_bytes[k] < 0 || info[k].stream < 0) continue;
        const int s = info[k].stream;
        if (s >= d.nstreams) {
            status[d.nstreams]++;
            continue;
        }
        const int slot = m->count[s]++;
        if (slot < d.max_rows) m->rows[(size_t)s * d.max_rows + slot] = k;
    }
    long long at_out = 0;
    for (int s = 0; s < d.nstreams; s++) {
        uint8_t *lac = m->lacing + (size_t)s * d.lace_cap, *q = m->body + (size_t)s * m->qstride;
        long long *gr = m->gran + (size_t)s * d.lace_cap;
        const int *rows = m->rows + (size_t)s * d.max_rows;
        const OggMuxPage *pages = m->pages + (size_t)s * d.max_pages;
        OggMuxHead &h = m->head[s];
        OggMuxCall &c = m->call[s];
        const int cnt = m->count[s];
        m->count[s] = 0;
        status[s] = oggmux_plan_stream(d, h, lac, gr, m->rows + (size_t)s * d.max_rows, cnt, packet_bytes, info,
                                       flush ? 1 : 0, m->pages + (size_t)s * d.max_pages, c);
        offsets[s] = at_out;
        // byte v of the virtual body
        std::vector<int> off(c.nrows + 2);
        off[0] = 0;
        int at = c.nbody_old;
        for (int j = 0; j < c.nrows; j++) {
            off[j + 1] = at;
            at += packet_bytes[rows[j]];
        }
        off[c.nrows + 1] = at;
        auto gather = [&](uint8_t *dst, int v, int n) {
            for (int k = 0; k <= c.nrows && n > 0; k++) {
                if (off[k + 1] <= v) continue;
                const int take = std::min(n, off[k + 1] - v);
                const uint8_t *src = k == 0 ? q : packets + (size_t)rows[k - 1] * packet_stride;
                memmove(dst, src + (v - off[k]), take);
                dst += take, v += take, n -= take;
            }
        };
        for (int p = 0; p < c.npages; p++) {
            const OggMuxPage &pg = pages[p];
            const long long L = 27 + pg.nseg + pg.body_bytes;
            if (at_out + L > out_capacity) return fail(VBM_EFAULT, "vbm_host_ogg_mux_packets: output bound exceeded");
            uint8_t *o = out + at_out;
            oggmux_page_header(pg, h.serialno, o);
            memcpy(o + 27, lac + pg.lace_at, pg.nseg);
            gather(o + 27 + pg.nseg, pg.body_at, pg.body_bytes);
            uint32_t crc = 0;
            for (long long i = 0; i < L; i++) crc = (crc << 8) ^ T.t[((crc >> 24) & 0xff) ^ o[i]];
            for (int i = 0; i < 4; i++) o[22 + i] = (uint8_t)((crc >> (8 * i)) & 0xff);
            at_out += L;
        }
        if (c.npages || c.nrows) {
            const int keep_body = c.body_total - c.body_used, keep = c.lace_total - c.lace_used;
            std::vector<uint8_t> rest((size_t)keep_body);
            gather(rest.data(), c.body_used, keep_body);
            if (keep_body) memcpy(q, rest.data(), keep_body);
            memmove(lac, lac + c.lace_used, keep);
            memmove(gr, gr + c.lace_used, sizeof(long long) * keep);
            h.nseg = keep;
            h.nbody = keep_body;
        }
    }
    offsets[d.nstreams] = at_out;
    return VBM_OK;
}
