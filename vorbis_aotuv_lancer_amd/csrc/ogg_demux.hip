// Ogg demux on the device for many whole files per call (rules, workspace and device helpers: ogg_demux.h), its host
// twin, and the C ABI over both (include/vorbis_mi355x.h, "Ogg demux, batch form"; host scaffold: twin_host.h).
//
//   scan:  k_dmx_walk        one lane per file: page after page, every header checked against the file's end before it
//                            is read; records each page's start and the body bytes / packets in front of it
//          k_dmx_scan_pages  one block, four files per thread: exclusive scan of the page counts -> dense page numbers
//          k_dmx_crc         one wavefront per page: 64 contiguous chunks, combined by the linearity of the code
//                            (dmx_wave_page_crc); a bad page marks its file
//          k_dmx_scan_info   one block: final status per file, exclusive scans of packets / payload / header bytes
//   fill:  k_dmx_fill        one wavefront per page: four lacing values per lane, a wave prefix sum gives every packet
//                            end its CSR slot; then the body goes to the headers and the payload (dword stores;
//                            misaligned sources through two aligned loads and a funnel shift)
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>
#include <string>

#include "ogg_demux.h"
#include "twin_host.h"

namespace {

constexpr int kPageBlocks = 2048;  // most blocks (of four wavefronts) a page-parallel kernel is launched with

// ---- kernels ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(64) k_dmx_walk(int nfiles, const uint8_t *data, const long long *off,
                                                 OggDmxPage *pages, vbm_ogg_file_info *info, long long *npages,
                                                 int *crc_bad)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nfiles) return;
    OggDmxWalk w;
    oggdmx_walk_begin(w, off[f], off[f + 1]);
    const long long slot = oggdmx_first_slot(off, f), room = oggdmx_first_slot(off, f + 1) - slot;
    OggDmxPage pg;
    int n = 0, rc;
    while ((rc = oggdmx_walk_step(data, w, pg)) == 1) {
        if (n >= room) {                            // cannot happen (a page is 27 bytes or more): second line of defence
            rc = -1;
            break;
        }
        pages[slot + n++] = pg;
    }
    vbm_ogg_file_info fi;
    oggdmx_walk_end(w, rc == 0, n, fi);
    info[f] = fi;
    npages[f] = fi.pages;
    crc_bad[f] = 0;
}

__global__ void __launch_bounds__(256) k_dmx_scan_pages(int nfiles, const long long *npages, long long *page_base)
{
    __shared__ long long wave_sum[4];
    block_scan_array<1>(nfiles, npages, page_base, page_base + nfiles, wave_sum);
}

__global__ void __launch_bounds__(256) k_dmx_crc(int nfiles, OggMuxPow pw, const uint8_t *data, const long long *off,
                                                 const OggDmxPage *pages, const long long *page_base, int *crc_bad)
{
    __shared__ uint32_t T[256];
    T[threadIdx.x] = oggmux_crc_entry(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long total = page_base[nfiles], nwaves = (long long)gridDim.x * 4;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < total; p += nwaves) {
        long long k;
        const int f = oggdmx_entry_of_page(page_base, nfiles, p, k);
        const OggDmxPage pg = pages[oggdmx_first_slot(off, f) + k];
        const bool ok = dmx_wave_page_crc(T, pw, data + pg.at, pg.len, lane);
        if (lane == 0 && !ok) crc_bad[f] = 1;
    }
}

__global__ void __launch_bounds__(256) k_dmx_scan_info(int nfiles, vbm_ogg_file_info *info, const int *crc_bad,
                                                        vbm_ogg_file_info *out_info, long long *totals,
                                                        long long *out_totals)
{
    __shared__ long long wave_sum[4];
    long long packets = 0, payload = 0, header = 0;
    for (int base = 0; base < nfiles; base += 256) {
        const int f = base + threadIdx.x;
        vbm_ogg_file_info fi = {};
        if (f < nfiles) {
            fi = info[f];
            if (crc_bad[f]) oggdmx_fail_file(fi);
        }
        const long long hb = (long long)fi.header_bytes[0] + fi.header_bytes[1] + fi.header_bytes[2];
        fi.packet_base = block_exclusive(fi.packets, packets, wave_sum);
        fi.payload_base = block_exclusive(fi.payload_bytes, payload, wave_sum);
        fi.header_base = block_exclusive(hb, header, wave_sum);
        if (f < nfiles) {
            info[f] = fi;
            out_info[f] = fi;
        }
    }
    if (threadIdx.x == 0) {
        totals[0] = out_totals[0] = packets;
        totals[1] = out_totals[1] = payload;
        totals[2] = out_totals[2] = header;
    }
}

__global__ void __launch_bounds__(256) k_dmx_fill(int nfiles, const uint8_t *data, const long long *off,
                                                  const OggDmxPage *pages, const long long *page_base,
                                                  const vbm_ogg_file_info *info, const long long *totals,
                                                  long long packet_cap, long long payload_cap, long long header_cap,
                                                  OggDmxOut out, int *status)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (totals[0] > packet_cap || totals[1] > payload_cap || totals[2] > header_cap) {
        if (first) *status = VBM_OGG_DEMUX_ECAP;    // the batch does not fit: nothing is written
        return;
    }
    if (first) {
        *status = 0;
        out.offsets[0] = 0;
    }
    const int lane = threadIdx.x & 63;
    const long long total = page_base[nfiles], nwaves = (long long)gridDim.x * 4;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < total; p += nwaves) {
        long long k;
        const int f = oggdmx_entry_of_page(page_base, nfiles, p, k);
        const vbm_ogg_file_info fi = info[f];
        if (fi.status) continue;                    // its CRC failed after the walk had counted its pages
        OggDmxPageCtx c;
        oggdmx_page_ctx(data, pages[oggdmx_first_slot(off, f) + k], fi, c);
        dmx_wave_packet_ends(c, out, lane);
        const OggDmxSplit s = oggdmx_body_split(c, out);
        if (s.n_h) dmx_wave_copy(s.dst_h, s.src_h, (int)s.n_h, lane);
        if (s.n_p) dmx_wave_copy(s.dst_p, s.src_p, (int)s.n_p, lane);
    }
}

}  // namespace

// ---- host side (scaffold: twin_host.h) --------------------------------------------------------------------------

struct vbm_ogg_demuxer {
    bool host = false;
    int max_files = 0;
    long long max_bytes = 0, max_slots = 0;
    OggMuxPow pow;
    TwinMem mem;                         // owns the workspace
    long long *off = nullptr;            // [max_files + 1] the call's file offsets
    OggDmxPage *pages = nullptr;         // [max_slots]
    long long *npages = nullptr, *page_base = nullptr;   // [max_files], [max_files + 1]
    vbm_ogg_file_info *info = nullptr;   // [max_files]
    int *crc_bad = nullptr;              // [max_files]
    long long *totals = nullptr;         // [3]
    int *status = nullptr;               // the status word of the last fill
    ArgStage stage;                      // device demuxer: the file offsets go up through it, [max_files + 1]
    // the last scan
    bool scanned = false;
    int nfiles = 0;
    const uint8_t *data = nullptr;
    long long slots = 0;                 // page slots its files span
};

namespace {

int create(vbm_ogg_demuxer **out, int max_files, long long max_bytes, bool host)
{
    if (!out || max_files < 1 || max_bytes < 0)
        return fail(VBM_EINVAL, "vbm_ogg_demuxer_create: bad argument (max_files >= 1, max_bytes >= 0)");
    if (!host) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(VBM_ENODEV, "vbm_ogg_demuxer_create: no HIP device");
    }
    vbm_ogg_demuxer *m = new (std::nothrow) vbm_ogg_demuxer();
    if (!m) return fail(VBM_EFAULT, "vbm_ogg_demuxer_create: out of memory");
    m->host = m->mem.host = host;
    m->max_files = max_files;
    m->max_bytes = max_bytes;
    m->max_slots = max_bytes / 27 + 1;
    m->pow = oggmux_pow_table();
    const size_t F = (size_t)max_files;
    const char *who = "vbm_ogg_demuxer";
    int rc = m->mem.get(m->off, F + 1, who);
    if (!rc) rc = m->mem.get(m->pages, (size_t)m->max_slots, who);
    if (!rc) rc = m->mem.get(m->npages, F, who);
    if (!rc) rc = m->mem.get(m->page_base, F + 1, who);
    if (!rc) rc = m->mem.get(m->info, F, who);
    if (!rc) rc = m->mem.get(m->crc_bad, F, who);
    if (!rc) rc = m->mem.get(m->totals, 3, who);
    if (!rc) rc = m->mem.get(m->status, 1, who);
    if (!rc && !host) rc = m->stage.create((F + 1) * sizeof(long long), "vbm_ogg_demuxer_create: staging");
    if (rc) {
        vbm_ogg_demuxer_destroy(m);
        return rc;
    }
    *out = m;
    return VBM_OK;
}

int check_scan(const vbm_ogg_demuxer *m, bool host, int nfiles, const uint8_t *data, const long long *off,
               const vbm_ogg_file_info *info, const long long *totals, const char *who)
{
    if (int rc = check_kind(m, host, who, "demuxer")) return rc;
    if (nfiles < 0 || nfiles > m->max_files)
        return fail(VBM_EINVAL, std::string(who) + ": nfiles is negative or above max_files");
    if (!off || !totals || (nfiles && !info)) return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    if (off[0] < 0) return fail(VBM_EINVAL, std::string(who) + ": negative file offset");
    for (int f = 0; f < nfiles; f++)
        if (off[f + 1] < off[f]) return fail(VBM_EINVAL, std::string(who) + ": file offsets decrease");
    if (off[nfiles] - off[0] > m->max_bytes)
        return fail(VBM_EINVAL, std::string(who) + ": the files span " + std::to_string(off[nfiles] - off[0]) +
                                    " bytes, above max_bytes = " + std::to_string(m->max_bytes));
    if (off[nfiles] > off[0] && !data) return fail(VBM_EINVAL, std::string(who) + ": null data");
    return VBM_OK;
}

int check_fill(const vbm_ogg_demuxer *m, bool host, const uint8_t *headers, long long header_cap, const uint8_t *payload,
               long long payload_cap, const long long *offsets, const long long *granulepos, const uint8_t *eos,
               long long packet_cap, const char *who)
{
    if (int rc = check_kind(m, host, who, "demuxer")) return rc;
    if (!m->scanned) return fail(VBM_EINVAL, std::string(who) + ": no scan has been made on this demuxer");
    if (header_cap < 0 || payload_cap < 0 || packet_cap < 0) return fail(VBM_EINVAL, std::string(who) + ": negative capacity");
    if (!offsets || (header_cap && !headers) || (payload_cap && !payload) || (packet_cap && (!granulepos || !eos)))
        return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    return VBM_OK;
}

void remember(vbm_ogg_demuxer *m, int nfiles, const uint8_t *data, const long long *off)
{
    m->scanned = true;
    m->nfiles = nfiles;
    m->data = data;
    m->slots = (off[nfiles] - off[0]) / 27 + 1;
}

dim3 page_grid(const vbm_ogg_demuxer *m)
{
    const long long blocks = (m->slots + 3) / 4;
    return dim3((unsigned)(blocks < kPageBlocks ? blocks : kPageBlocks));
}

}  // namespace

extern "C" int vbm_ogg_demuxer_create(vbm_ogg_demuxer **dm, int max_files, long long max_bytes)
{
    return create(dm, max_files, max_bytes, false);
}

extern "C" int vbm_host_ogg_demuxer_create(vbm_ogg_demuxer **dm, int max_files, long long max_bytes)
{
    return create(dm, max_files, max_bytes, true);
}

extern "C" void vbm_ogg_demuxer_destroy(vbm_ogg_demuxer *m)
{
    if (!m) return;
    m->mem.free_all();
    m->stage.destroy();
    delete m;
}

extern "C" int vbm_ogg_demux_scan(vbm_ogg_demuxer *m, int nfiles, const uint8_t *d_data, const long long *file_offsets,
                                  vbm_ogg_file_info *d_info, long long *d_totals, void *stream)
{
    int rc = check_scan(m, false, nfiles, d_data, file_offsets, d_info, d_totals, "vbm_ogg_demux_scan");
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    const size_t off_bytes = ((size_t)nfiles + 1) * sizeof(long long);
    void *h_off;
    rc = m->stage.next(h_off, "vbm_ogg_demux_scan: hipEventSynchronize(stage)");
    if (rc) return rc;
    memcpy(h_off, file_offsets, off_bytes);
    rc = m->stage.send(m->off, off_bytes, q, "vbm_ogg_demux_scan: upload of the file offsets");
    if (rc) return rc;
    remember(m, nfiles, d_data, file_offsets);
    if (nfiles > 0)
        hipLaunchKernelGGL(k_dmx_walk, dim3((nfiles + 63) / 64), dim3(64), 0, q, nfiles, d_data, m->off, m->pages, m->info,
                           m->npages, m->crc_bad);
    hipLaunchKernelGGL(k_dmx_scan_pages, dim3(1), dim3(256), 0, q, nfiles, m->npages, m->page_base);
    if (nfiles > 0)
        hipLaunchKernelGGL(k_dmx_crc, page_grid(m), dim3(256), 0, q, nfiles, m->pow, d_data, m->off, m->pages,
                           m->page_base, m->crc_bad);
    hipLaunchKernelGGL(k_dmx_scan_info, dim3(1), dim3(256), 0, q, nfiles, m->info, m->crc_bad, d_info, m->totals,
                       d_totals);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_demux_scan: launch");
}

extern "C" int vbm_ogg_demux_fill(vbm_ogg_demuxer *m, uint8_t *d_headers, long long header_cap, uint8_t *d_payload,
                                  long long payload_cap, long long *d_offsets, long long *d_granulepos, uint8_t *d_eos,
                                  long long packet_cap, void *stream)
{
    int rc = check_fill(m, false, d_headers, header_cap, d_payload, payload_cap, d_offsets, d_granulepos, d_eos, packet_cap,
                        "vbm_ogg_demux_fill");
    if (rc) return rc;
    const OggDmxOut out = {d_headers, d_payload, d_offsets, d_granulepos, d_eos};
    hipLaunchKernelGGL(k_dmx_fill, page_grid(m), dim3(256), 0, (hipStream_t)stream, m->nfiles, m->data, m->off, m->pages,
                       m->page_base, m->info, m->totals, packet_cap, payload_cap, header_cap, out, m->status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_demux_fill: launch");
}

extern "C" int vbm_ogg_demux_status(vbm_ogg_demuxer *m, int *status, void *stream)
{
    if (!m || !status) return fail(VBM_EINVAL, "vbm_ogg_demux_status: null pointer");
    return read_status(m->host, m->status, status, stream, "vbm_ogg_demux_status");
}

// ---- the same on the CPU: the functions of ogg_demux.h, file after file and page after page ---------------------------
extern "C" int vbm_host_ogg_demux_scan(vbm_ogg_demuxer *m, int nfiles, const uint8_t *data, const long long *file_offsets,
                                       vbm_ogg_file_info *info, long long *totals)
{
    int rc = check_scan(m, true, nfiles, data, file_offsets, info, totals, "vbm_host_ogg_demux_scan");
    if (rc) return rc;
    const uint32_t *T = crc_table().t;
    memcpy(m->off, file_offsets, ((size_t)nfiles + 1) * sizeof(long long));
    remember(m, nfiles, data, file_offsets);
    long long npages = 0, packets = 0, payload = 0, header = 0;
    for (int f = 0; f < nfiles; f++) {
        OggDmxWalk w;
        oggdmx_walk_begin(w, m->off[f], m->off[f + 1]);
        OggDmxPage *pages = m->pages + oggdmx_first_slot(m->off, f);
        int n = 0, r;
        bool crc_ok = true;
        while ((r = oggdmx_walk_step(data, w, pages[n])) == 1) {
            crc_ok = crc_ok && oggdmx_page_crc_ok(T, m->pow, data + pages[n].at, pages[n].len);
            n++;
        }
        vbm_ogg_file_info fi;
        oggdmx_walk_end(w, r == 0 && crc_ok, n, fi);
        fi.packet_base = packets, fi.payload_base = payload, fi.header_base = header;
        packets += fi.packets;
        payload += fi.payload_bytes;
        header += (long long)fi.header_bytes[0] + fi.header_bytes[1] + fi.header_bytes[2];
        m->page_base[f] = npages;
        npages += fi.pages;
        m->info[f] = info[f] = fi;
    }
    m->page_base[nfiles] = npages;
    m->totals[0] = totals[0] = packets;
    m->totals[1] = totals[1] = payload;
    m->totals[2] = totals[2] = header;
    return VBM_OK;
}

extern "C" int vbm_host_ogg_demux_fill(vbm_ogg_demuxer *m, uint8_t *headers, long long header_cap, uint8_t *payload,
                                       long long payload_cap, long long *offsets, long long *granulepos, uint8_t *eos,
                                       long long packet_cap)
{
    int rc = check_fill(m, true, headers, header_cap, payload, payload_cap, offsets, granulepos, eos, packet_cap,
                        "vbm_host_ogg_demux_fill");
    if (rc) return rc;
    if (m->totals[0] > packet_cap || m->totals[1] > payload_cap || m->totals[2] > header_cap) {
        *m->status = VBM_OGG_DEMUX_ECAP;
        return VBM_OK;
    }
    *m->status = 0;
    const OggDmxOut out = {headers, payload, offsets, granulepos, eos};
    offsets[0] = 0;
    for (int f = 0; f < m->nfiles; f++) {
        const vbm_ogg_file_info &fi = m->info[f];
        const OggDmxPage *pages = m->pages + oggdmx_first_slot(m->off, f);
        for (int p = 0; p < fi.pages; p++) {
            OggDmxPageCtx c;
            oggdmx_page_ctx(m->data, pages[p], fi, c);
            oggdmx_page_packet_ends(c, out);
            const OggDmxSplit s = oggdmx_body_split(c, out);
            if (s.n_h) memcpy(s.dst_h, s.src_h, (size_t)s.n_h);
            if (s.n_p) memcpy(s.dst_p, s.src_p, (size_t)s.n_p);
        }
    }
    return VBM_OK;
}
