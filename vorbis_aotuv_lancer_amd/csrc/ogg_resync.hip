// Tolerant Ogg demux on the device for many whole files per call (rule, records and workspace: ogg_resync.h), its host
// twin, and the C ABI over both (include/vorbis_mi355x.h, "Tolerant Ogg demux"; host scaffold: twin_host.h).
//
//   scan:  k_rs_count         the capture search, byte-parallel over the joined buffer: a tile is 16 KB of aligned dwords,
//                             a lane tests the 16 windows that start in its four dwords (a fifth, the next lane's first,
//                             completes the last three); a hit counts when its four bytes lie in one file -> hits per tile
//          k_rs_scan_tiles    one block: exclusive scan of the tile counts -> where each tile's candidates go, the total
//          k_rs_write         the search again: a block scan per row gives every hit its place, in position order
//          k_rs_judge         one wavefront per candidate: header bytes and lacing values in one round trip, none outside
//                             the candidate's file; version, claimed size, "runs past the file's end"; the CRC of a whole
//                             candidate (dmx_wave_page_crc); a wave scan gives the summary of the lacing table
//          k_rs_resolve       one lane per file over its candidate records (oggrs_resolve_file): page records, side
//                             records, entries, events
//          k_rs_scan_files    one block: exclusive scans of the files' entries (-> d_file_links) and pages
//          k_rs_scan_entries  one block: the entries densely, exclusive scans of packets / payload / header bytes, totals
//   fill:  k_rs_fill          one wavefront per page, as k_dmx_fill, behind the segments that belong to no packet and
//                             clipped where a discontinuity dropped a packet; writes the gap marks too
// The scans of ogg_demux.hip are one block_scan_array call each and k_dmx_fill finds a page's slot from the file offsets
// alone, so this file has kernels of its own over the same helpers and no strict kernel is touched.
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>
#include <string>

#include "ogg_resync.h"
#include "twin_host.h"

namespace {

constexpr int kSearchBlocks = 1024;  // most blocks the search is launched with (grid-stride over tiles)
constexpr int kWaveBlocks = 2048;    // most blocks (of four wavefronts) a candidate- or page-parallel kernel is launched with

enum { CTL_NCAND = 0, CTL_ENTRIES, CTL_PACKETS, CTL_PAYLOAD, CTL_HEADER, CTL_N };

struct RsSpan {                      // the joined buffer as aligned dwords
    const uint32_t *A;               // the dword that holds the first byte
    long long nd, n, off0;           // dwords that hold a byte of it, its bytes, its first byte in the call's data
    int mis;                         // bytes of A[0] in front of it
};

// ---- kernels ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ RsSpan rs_span(const uint8_t *data, const long long *off, int nfiles)
{
    RsSpan s;
    s.off0 = off[0];
    s.n = off[nfiles] - s.off0;
    const uint8_t *d0 = data + s.off0;
    s.mis = (int)((uintptr_t)d0 & 3);
    s.A = (const uint32_t *)(d0 - s.mis);
    s.nd = (s.mis + s.n + 3) >> 2;
    return s;
}

// where in the joined buffer the window at byte j of dword w starts
__device__ __forceinline__ long long rs_window_at(const RsSpan &s, long long w, int j) { return 4 * w + j - s.mis; }

// The hits among the 16 windows that start in dwords [w0, w0 + 4): bit 4 k + j = byte j of dword w0 + k.  Only dwords
// that hold a byte of the buffer are loaded, and a window counts only when all of it lies in the buffer and in one file.
__device__ __forceinline__ uint32_t rs_row_hits(const RsSpan &s, long long w0, const long long *off, int nfiles)
{
    uint32_t d[5];
#pragma unroll
    for (int k = 0; k < 5; k++) d[k] = w0 + k < s.nd ? s.A[w0 + k] : 0u;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = j ? (d[k] >> (8 * j)) | (d[k + 1] << (32 - 8 * j)) : d[k];
            if (!oggrs_capture(v)) continue;
            const long long p = rs_window_at(s, w0 + k, j);
            if (p < 0 || p + 4 > s.n) continue;
            const int f = oggdmx_file_of_page(off, nfiles, s.off0 + p);
            if (s.off0 + p + 4 <= off[f + 1]) m |= 1u << (4 * k + j);
        }
    }
    return m;
}

__global__ void __launch_bounds__(256) k_rs_count(int nfiles, const uint8_t *data, const long long *off, int ntiles,
                                                  long long *tile_count)
{
    __shared__ long long wave_sum[4];
    const RsSpan s = rs_span(data, off, nfiles);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int c = 0;
        for (int r = 0; r < 4; r++)
            c += __popc(rs_row_hits(s, (long long)t * kRsTileDwords + r * kRsRowDwords + threadIdx.x * 4, off, nfiles));
        long long carry = 0;
        block_exclusive(c, carry, wave_sum);
        if (threadIdx.x == 0) tile_count[t] = carry;
    }
}

__global__ void __launch_bounds__(256) k_rs_scan_tiles(int ntiles, const long long *tile_count, long long *tile_base,
                                                       long long *ctl)
{
    __shared__ long long wave_sum[4];
    block_scan_array<1>(ntiles, tile_count, tile_base, ctl + CTL_NCAND, wave_sum);
}

__global__ void __launch_bounds__(256) k_rs_write(int nfiles, const uint8_t *data, const long long *off, int ntiles,
                                                  const long long *tile_base, const long long *ctl, long long max_cand,
                                                  OggRsCand *cand)
{
    __shared__ long long wave_sum[4];
    if (ctl[CTL_NCAND] > max_cand) return;          // they do not fit: nothing is written
    const RsSpan s = rs_span(data, off, nfiles);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        long long carry = tile_base[t];
        for (int r = 0; r < 4; r++) {
            const long long w0 = (long long)t * kRsTileDwords + r * kRsRowDwords + threadIdx.x * 4;
            uint32_t m = rs_row_hits(s, w0, off, nfiles);
            long long at = block_exclusive(__popc(m), carry, wave_sum);
            while (m) {
                const int b = __ffs(m) - 1;
                m &= m - 1;
                const long long p = s.off0 + rs_window_at(s, w0 + (b >> 2), b & 3);
                cand[at].at = p;
                cand[at].file = oggdmx_file_of_page(off, nfiles, p);
                at++;
            }
        }
    }
}

__device__ __forceinline__ int rs_wave_max(int v)
{
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

// The candidate at `at` of file `file`, which ends at file_end, by the 64 lanes of a wavefront (the host's: oggrs_judge).
// Every value a decision hangs on is uniform over the wavefront.  Lane 0 writes the record.
__device__ __forceinline__ void rs_wave_judge(const uint32_t *T, const OggMuxPow &pw, const uint8_t *data, long long file_end,
                                              long long at, int file, OggRsCand *out, int lane)
{
    const uint8_t *h = data + at;
    const long long left = file_end - at;
    // the round trip: header byte `lane`, and lacing values 4 * lane .. 4 * lane + 3, as far as the file goes
    const int hb = (lane < 27 && lane < left) ? h[lane] : 0;
    const uint32_t lw = dmx_load4(h + 27 + 4 * lane, left - 27 - 4 * lane);
    const int version = __builtin_amdgcn_readlane(hb, 4), flags = __builtin_amdgcn_readlane(hb, 5);
    const int nseg = __builtin_amdgcn_readlane(hb, 26);
    OggRsCand c = {};
    c.at = at;
    c.file = file;
    c.verdict = OGGRS_NO;
    if (!(left >= 5 && version != 0)) {
        c.verdict = OGGRS_END;
        if (left >= 27 && left - 27 >= nseg) {
            // bytes (<= 65025) and packet ends (<= 255) of a page share one word, as in dmx_wave_packet_ends
            int lv[4], mine = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                lv[j] = lane * 4 + j < nseg ? (int)((lw >> (8 * j)) & 0xff) : -1;
                if (lv[j] >= 0) mine += lv[j] + (lv[j] < 255 ? 1 << 20 : 0);
            }
            int x = mine;
            for (int dist = 1; dist < 64; dist <<= 1) {
                const int y = __shfl_up(x, dist, 64);
                if (lane >= dist) x += y;
            }
            const int total = __builtin_amdgcn_readlane(x, 63);
            const int body = total & 0xfffff, nends = total >> 20;
            if (left - 27 - nseg >= body) {
                int bytes = (x - mine) & 0xfffff, ends = (x - mine) >> 20;
                int e0 = 0, e1 = 0, e2 = 0, last_end = 0, partial = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (lv[j] < 0) continue;
                    bytes += lv[j];
                    if (lv[j] < 255) {
                        if (ends == 0) e0 = bytes;
                        if (ends == 1) e1 = bytes;
                        if (ends == 2) e2 = bytes;
                        ends++;
                        last_end = bytes;
                    }
                    if (lane * 4 + j == nseg - 1) partial = lv[j] == 255;
                }
                c.e0 = rs_wave_max(e0), c.e1 = rs_wave_max(e1), c.e2 = rs_wave_max(e2);
                c.last_end = rs_wave_max(last_end);
                c.partial = (uint8_t)rs_wave_max(partial);
                c.nseg = (uint8_t)nseg;
                c.body = body;
                c.nends = nends;
                c.len = 27 + nseg + body;
                c.flags = (uint8_t)flags;
                c.serial = (uint32_t)__builtin_amdgcn_readlane(hb, 14) | ((uint32_t)__builtin_amdgcn_readlane(hb, 15) << 8) |
                           ((uint32_t)__builtin_amdgcn_readlane(hb, 16) << 16) | ((uint32_t)__builtin_amdgcn_readlane(hb, 17) << 24);
                c.seq = (uint32_t)__builtin_amdgcn_readlane(hb, 18) | ((uint32_t)__builtin_amdgcn_readlane(hb, 19) << 8) |
                        ((uint32_t)__builtin_amdgcn_readlane(hb, 20) << 16) | ((uint32_t)__builtin_amdgcn_readlane(hb, 21) << 24);
                c.verdict = dmx_wave_page_crc(T, pw, h, c.len, lane) ? OGGRS_GOOD : OGGRS_NO;
            }
        }
    }
    if (lane == 0) *out = c;
}

__global__ void __launch_bounds__(256) k_rs_judge(OggMuxPow pw, const uint8_t *data, const long long *off,
                                                  const long long *ctl, long long max_cand, OggRsCand *cand)
{
    __shared__ uint32_t T[256];
    T[threadIdx.x] = oggmux_crc_entry(threadIdx.x);
    __syncthreads();
    const long long total = ctl[CTL_NCAND], nwaves = (long long)gridDim.x * 4;
    if (total > max_cand) return;
    const int lane = threadIdx.x & 63;
    for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < total; i += nwaves) {
        const long long at = cand[i].at;
        const int file = cand[i].file;
        rs_wave_judge(T, pw, data, off[file + 1], at, file, cand + i, lane);
    }
}

__global__ void __launch_bounds__(64) k_rs_resolve(int nfiles, const long long *off, const long long *ctl, long long max_cand,
                                                   const OggRsCand *cand, OggDmxPage *pages, OggRsSide *side,
                                                   vbm_ogg_file_info *ent, long long *npages, long long *nent,
                                                   long long *cand_lo, vbm_ogg_resync_events *events)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    const long long total = ctl[CTL_NCAND];
    if (f >= nfiles || total > max_cand) return;
    const long long lo = oggrs_lower_bound(cand, total, off[f]), hi = oggrs_lower_bound(cand, total, off[f + 1]);
    long long np, ne;
    vbm_ogg_resync_events ev;
    oggrs_resolve_file(cand + lo, hi - lo, off[f], off[f + 1], pages + lo, side + lo, ent + lo, np, ne, ev);
    npages[f] = np;
    nent[f] = ne;
    cand_lo[f] = lo;
    events[f] = ev;
}

__global__ void __launch_bounds__(256) k_rs_scan_files(int nfiles, const long long *ctl, long long max_cand,
                                                       const long long *npages, const long long *nent, long long *page_base,
                                                       long long *file_links, long long *out_file_links)
{
    __shared__ long long wave_sum[4];
    if (ctl[CTL_NCAND] > max_cand) return;
    block_scan_array<1>(nfiles, npages, page_base, page_base + nfiles, wave_sum);
    block_scan_array<1>(nfiles, nent, file_links, file_links + nfiles, wave_sum);
    block_scan_array<1>(nfiles, nent, out_file_links, out_file_links + nfiles, wave_sum);
}

__global__ void __launch_bounds__(256) k_rs_scan_entries(int nfiles, long long *ctl, long long max_cand,
                                                         const long long *file_links, const long long *cand_lo,
                                                         const vbm_ogg_file_info *ent, vbm_ogg_file_info *info,
                                                         vbm_ogg_file_info *out_info, long long entry_cap,
                                                         long long *out_totals, int *st)
{
    __shared__ long long wave_sum[4];
    const long long ncand = ctl[CTL_NCAND];
    if (ncand > max_cand) {
        if (threadIdx.x == 0) {
            out_totals[4] = ncand;
            out_totals[5] = VBM_OGG_DEMUX_ECAP;
            st[0] = st[1] = VBM_OGG_DEMUX_ECAP;
        }
        return;
    }
    const long long total = file_links[nfiles];
    const bool fits = total <= entry_cap;
    long long packets = 0, payload = 0, header = 0;
    for (long long base = 0; base < total; base += 256) {
        const long long j = base + threadIdx.x;
        vbm_ogg_file_info fi = {};
        if (j < total) {
            const int f = oggdmx_file_of_page(file_links, nfiles, j);
            fi = ent[cand_lo[f] + (j - file_links[f])];
        }
        const long long hb = (long long)fi.header_bytes[0] + fi.header_bytes[1] + fi.header_bytes[2];
        fi.packet_base = block_exclusive(fi.packets, packets, wave_sum);
        fi.payload_base = block_exclusive(fi.payload_bytes, payload, wave_sum);
        fi.header_base = block_exclusive(hb, header, wave_sum);
        if (j < total) {
            info[j] = fi;
            if (fits) out_info[j] = fi;
        }
    }
    if (threadIdx.x == 0) {
        ctl[CTL_ENTRIES] = out_totals[0] = total;
        ctl[CTL_PACKETS] = out_totals[1] = packets;
        ctl[CTL_PAYLOAD] = out_totals[2] = payload;
        ctl[CTL_HEADER] = out_totals[3] = header;
        out_totals[4] = ncand;
        out_totals[5] = st[0] = st[1] = fits ? 0 : VBM_OGG_DEMUX_ECAP;
    }
}

__global__ void __launch_bounds__(256) k_rs_fill(int nfiles, const uint8_t *data, const OggDmxPage *pages, const OggRsSide *side,
                                                 const long long *page_base, const long long *file_links,
                                                 const long long *cand_lo, const vbm_ogg_file_info *info, const long long *ctl,
                                                 long long packet_cap, long long payload_cap, long long header_cap,
                                                 OggDmxOut out, uint8_t *gap, int *st)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (st[0] || ctl[CTL_PACKETS] > packet_cap || ctl[CTL_PAYLOAD] > payload_cap || ctl[CTL_HEADER] > header_cap) {
        if (first) st[1] = VBM_OGG_DEMUX_ECAP;      // the batch does not fit: nothing is written
        return;
    }
    if (first) {
        st[1] = 0;
        out.offsets[0] = 0;
    }
    const int lane = threadIdx.x & 63;
    const long long total = page_base[nfiles], nwaves = (long long)gridDim.x * 4;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < total; p += nwaves) {
        long long k;
        const int f = oggdmx_entry_of_page(page_base, nfiles, p, k);
        const long long slot = cand_lo[f] + k;
        const OggRsSide sd = side[slot];
        OggDmxPageCtx c;
        oggrs_page_ctx(data, pages[slot], sd, info[file_links[f] + sd.entry], c);
        dmx_wave_packet_ends(c, out, lane);
        long long g0, g1;
        oggrs_gap_range(c, sd, g0, g1);
        for (long long q = g0 + lane; q < g1; q += 64) gap[c.packet_base + q] = q == sd.gap_pkt ? 1 : 0;
        const OggDmxSplit s = oggrs_body_split(c, sd, out);
        if (s.n_h) dmx_wave_copy(s.dst_h, s.src_h, (int)s.n_h, lane);
        if (s.n_p) dmx_wave_copy(s.dst_p, s.src_p, (int)s.n_p, lane);
    }
}

}  // namespace

// ---- host side (scaffold: twin_host.h) --------------------------------------------------------------------------

struct vbm_ogg_resync {
    bool host = false;
    int max_files = 0;
    long long max_bytes = 0, max_cand = 0, max_tiles = 0;
    OggMuxPow pow;
    TwinMem mem;                         // owns the workspace
    long long *off = nullptr;            // [max_files + 1] the call's file offsets
    long long *tile_count = nullptr, *tile_base = nullptr;   // [max_tiles + 1]
    OggRsCand *cand = nullptr;           // [max_cand]
    OggDmxPage *pages = nullptr;         // [max_cand] file f's from cand_lo[f] on, as its side records and entries
    OggRsSide *side = nullptr;           // [max_cand]
    vbm_ogg_file_info *ent = nullptr;    // [max_cand] the entries as the resolve leaves them
    vbm_ogg_file_info *info = nullptr;   // [max_cand] ... dense, with their bases
    long long *npages = nullptr, *nent = nullptr, *cand_lo = nullptr;   // [max_files]
    long long *page_base = nullptr, *file_links = nullptr;               // [max_files + 1]
    long long *ctl = nullptr;            // [CTL_N] candidates, entries, packets, payload bytes, header bytes
    int *st = nullptr;                   // [2] the status of the last scan, the status word
    ArgStage stage;                      // device form: the file offsets go up through it, [max_files + 1]
    // the last scan
    bool scanned = false;
    int nfiles = 0;
    const uint8_t *data = nullptr;
    long long span = 0;
};

namespace {

int create(vbm_ogg_resync **out, int max_files, long long max_bytes, long long max_cand, bool host)
{
    if (!out || max_files < 1 || max_bytes < 0 || max_cand < 0)
        return fail(VBM_EINVAL, "vbm_ogg_resync_create: bad argument (max_files >= 1, max_bytes >= 0, max_candidates >= 0)");
    if (!host) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(VBM_ENODEV, "vbm_ogg_resync_create: no HIP device");
    }
    vbm_ogg_resync *m = new (std::nothrow) vbm_ogg_resync();
    if (!m) return fail(VBM_EFAULT, "vbm_ogg_resync_create: out of memory");
    m->host = m->mem.host = host;
    m->max_files = max_files;
    m->max_bytes = max_bytes;
    m->max_cand = max_cand;
    m->max_tiles = (max_bytes + 6) / 4 / kRsTileDwords + 1;
    m->pow = oggmux_pow_table();
    const size_t F = (size_t)max_files, K = (size_t)max_cand;
    const char *who = "vbm_ogg_resync";
    int rc = m->mem.get(m->off, F + 1, who);
    if (!rc && !host) rc = m->mem.get(m->tile_count, (size_t)m->max_tiles + 1, who);
    if (!rc && !host) rc = m->mem.get(m->tile_base, (size_t)m->max_tiles + 1, who);
    if (!rc) rc = m->mem.get(m->cand, K, who);
    if (!rc) rc = m->mem.get(m->pages, K, who);
    if (!rc) rc = m->mem.get(m->side, K, who);
    if (!rc) rc = m->mem.get(m->ent, K, who);
    if (!rc) rc = m->mem.get(m->info, K, who);
    if (!rc) rc = m->mem.get(m->npages, F, who);
    if (!rc) rc = m->mem.get(m->nent, F, who);
    if (!rc) rc = m->mem.get(m->cand_lo, F, who);
    if (!rc) rc = m->mem.get(m->page_base, F + 1, who);
    if (!rc) rc = m->mem.get(m->file_links, F + 1, who);
    if (!rc) rc = m->mem.get(m->ctl, CTL_N, who);
    if (!rc) rc = m->mem.get(m->st, 2, who);
    if (!rc && !host) rc = m->stage.create((F + 1) * sizeof(long long), "vbm_ogg_resync_create: staging");
    if (rc) {
        vbm_ogg_resync_destroy(m);
        return rc;
    }
    *out = m;
    return VBM_OK;
}

int check_scan(const vbm_ogg_resync *m, bool host, int nfiles, const uint8_t *data, const long long *off,
               const vbm_ogg_resync_events *events, const long long *file_links, const vbm_ogg_file_info *info,
               long long entry_cap, const long long *totals, const char *who)
{
    if (int rc = check_kind(m, host, who, "resync")) return rc;
    if (nfiles < 0 || nfiles > m->max_files)
        return fail(VBM_EINVAL, std::string(who) + ": nfiles is negative or above max_files");
    if (entry_cap < 0) return fail(VBM_EINVAL, std::string(who) + ": negative capacity");
    if (!off || !totals || !file_links || (nfiles && !events) || (entry_cap && !info))
        return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    if (off[0] < 0) return fail(VBM_EINVAL, std::string(who) + ": negative file offset");
    for (int f = 0; f < nfiles; f++)
        if (off[f + 1] < off[f]) return fail(VBM_EINVAL, std::string(who) + ": file offsets decrease");
    if (off[nfiles] - off[0] > m->max_bytes)
        return fail(VBM_EINVAL, std::string(who) + ": the files span " + std::to_string(off[nfiles] - off[0]) +
                                    " bytes, above max_bytes = " + std::to_string(m->max_bytes));
    if (off[nfiles] > off[0] && !data) return fail(VBM_EINVAL, std::string(who) + ": null data");
    return VBM_OK;
}

int check_fill(const vbm_ogg_resync *m, bool host, const uint8_t *headers, long long header_cap, const uint8_t *payload,
               long long payload_cap, const long long *offsets, const long long *granulepos, const uint8_t *eos,
               const uint8_t *gap, long long packet_cap, const char *who)
{
    if (int rc = check_kind(m, host, who, "resync")) return rc;
    if (!m->scanned) return fail(VBM_EINVAL, std::string(who) + ": no scan has been made on this object");
    if (header_cap < 0 || payload_cap < 0 || packet_cap < 0) return fail(VBM_EINVAL, std::string(who) + ": negative capacity");
    if (!offsets || (header_cap && !headers) || (payload_cap && !payload) || (packet_cap && (!granulepos || !eos || !gap)))
        return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    return VBM_OK;
}

void remember(vbm_ogg_resync *m, int nfiles, const uint8_t *data, const long long *off)
{
    m->scanned = true;
    m->nfiles = nfiles;
    m->data = data;
    m->span = off[nfiles] - off[0];
}

// blocks of four wavefronts for up to `most` items, one wavefront each
dim3 wave_grid(long long most)
{
    const long long blocks = (most + 3) / 4;
    return dim3((unsigned)(blocks < 1 ? 1 : blocks < kWaveBlocks ? blocks : kWaveBlocks));
}

}  // namespace

extern "C" int vbm_ogg_resync_create(vbm_ogg_resync **rs, int max_files, long long max_bytes, long long max_candidates)
{
    return create(rs, max_files, max_bytes, max_candidates, false);
}

extern "C" int vbm_host_ogg_resync_create(vbm_ogg_resync **rs, int max_files, long long max_bytes, long long max_candidates)
{
    return create(rs, max_files, max_bytes, max_candidates, true);
}

extern "C" void vbm_ogg_resync_destroy(vbm_ogg_resync *m)
{
    if (!m) return;
    m->mem.free_all();
    m->stage.destroy();
    delete m;
}

extern "C" int vbm_ogg_resync_scan(vbm_ogg_resync *m, int nfiles, const uint8_t *d_data, const long long *file_offsets,
                                   vbm_ogg_resync_events *d_events, long long *d_file_links, vbm_ogg_file_info *d_info,
                                   long long entry_cap, long long *d_totals, void *stream)
{
    int rc = check_scan(m, false, nfiles, d_data, file_offsets, d_events, d_file_links, d_info, entry_cap, d_totals,
                        "vbm_ogg_resync_scan");
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    const size_t off_bytes = ((size_t)nfiles + 1) * sizeof(long long);
    void *h_off;
    rc = m->stage.next(h_off, "vbm_ogg_resync_scan: hipEventSynchronize(stage)");
    if (rc) return rc;
    memcpy(h_off, file_offsets, off_bytes);
    rc = m->stage.send(m->off, off_bytes, q, "vbm_ogg_resync_scan: upload of the file offsets");
    if (rc) return rc;
    remember(m, nfiles, d_data, file_offsets);
    // the tiles of the joined buffer, counted from the dword that holds its first byte (rs_span)
    const long long n = m->span, mis = n ? (long long)((uintptr_t)(d_data + file_offsets[0]) & 3) : 0;
    const int ntiles = (int)(((mis + n + 3) / 4 + kRsTileDwords - 1) / kRsTileDwords);
    const dim3 search((unsigned)(ntiles < 1 ? 1 : ntiles < kSearchBlocks ? ntiles : kSearchBlocks));
    const long long most_cand = m->max_cand < n / 4 ? m->max_cand : n / 4;
    const dim3 files((unsigned)((nfiles + 63) / 64 < 1 ? 1 : (nfiles + 63) / 64));
    hipLaunchKernelGGL(k_rs_count, search, dim3(256), 0, q, nfiles, d_data, m->off, ntiles, m->tile_count);
    hipLaunchKernelGGL(k_rs_scan_tiles, dim3(1), dim3(256), 0, q, ntiles, m->tile_count, m->tile_base, m->ctl);
    hipLaunchKernelGGL(k_rs_write, search, dim3(256), 0, q, nfiles, d_data, m->off, ntiles, m->tile_base, m->ctl, m->max_cand,
                       m->cand);
    hipLaunchKernelGGL(k_rs_judge, wave_grid(most_cand), dim3(256), 0, q, m->pow, d_data, m->off, m->ctl, m->max_cand,
                       m->cand);
    hipLaunchKernelGGL(k_rs_resolve, files, dim3(64), 0, q, nfiles, m->off, m->ctl, m->max_cand, m->cand, m->pages, m->side,
                       m->ent, m->npages, m->nent, m->cand_lo, d_events);
    hipLaunchKernelGGL(k_rs_scan_files, dim3(1), dim3(256), 0, q, nfiles, m->ctl, m->max_cand, m->npages, m->nent,
                       m->page_base, m->file_links, d_file_links);
    hipLaunchKernelGGL(k_rs_scan_entries, dim3(1), dim3(256), 0, q, nfiles, m->ctl, m->max_cand, m->file_links, m->cand_lo,
                       m->ent, m->info, d_info, entry_cap, d_totals, m->st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_resync_scan: launch");
}

extern "C" int vbm_ogg_resync_fill(vbm_ogg_resync *m, uint8_t *d_headers, long long header_cap, uint8_t *d_payload,
                                   long long payload_cap, long long *d_offsets, long long *d_granulepos, uint8_t *d_eos,
                                   uint8_t *d_gap, long long packet_cap, void *stream)
{
    int rc = check_fill(m, false, d_headers, header_cap, d_payload, payload_cap, d_offsets, d_granulepos, d_eos, d_gap,
                        packet_cap, "vbm_ogg_resync_fill");
    if (rc) return rc;
    const OggDmxOut out = {d_headers, d_payload, d_offsets, d_granulepos, d_eos};
    const long long most_pages = m->max_cand < m->span / 27 + 1 ? m->max_cand : m->span / 27 + 1;
    hipLaunchKernelGGL(k_rs_fill, wave_grid(most_pages), dim3(256), 0, (hipStream_t)stream, m->nfiles, m->data, m->pages,
                       m->side, m->page_base, m->file_links, m->cand_lo, m->info, m->ctl, packet_cap, payload_cap,
                       header_cap, out, d_gap, m->st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_resync_fill: launch");
}

extern "C" int vbm_ogg_resync_status(vbm_ogg_resync *m, int *status, void *stream)
{
    if (!m || !status) return fail(VBM_EINVAL, "vbm_ogg_resync_status: null pointer");
    return read_status(m->host, m->st + 1, status, stream, "vbm_ogg_resync_status");
}

// ---- the same on the CPU: the functions of ogg_resync.h, file after file and candidate after candidate ------------------
extern "C" int vbm_host_ogg_resync_scan(vbm_ogg_resync *m, int nfiles, const uint8_t *data, const long long *file_offsets,
                                        vbm_ogg_resync_events *events, long long *file_links, vbm_ogg_file_info *info,
                                        long long entry_cap, long long *totals)
{
    int rc = check_scan(m, true, nfiles, data, file_offsets, events, file_links, info, entry_cap, totals,
                        "vbm_host_ogg_resync_scan");
    if (rc) return rc;
    const uint32_t *T = crc_table().t;
    memcpy(m->off, file_offsets, ((size_t)nfiles + 1) * sizeof(long long));
    remember(m, nfiles, data, file_offsets);
    // the capture search: every pattern whose four bytes lie in one file, in position order
    long long ncand = 0;
    for (int f = 0; f < nfiles; f++)
        for (long long p = m->off[f]; p + 4 <= m->off[f + 1]; p++) {
            if (!oggrs_capture(oggdmx_rd32(data + p))) continue;
            if (ncand < m->max_cand) m->cand[ncand].at = p, m->cand[ncand].file = f;
            ncand++;
        }
    m->ctl[CTL_NCAND] = ncand;
    if (ncand > m->max_cand) {
        totals[4] = ncand;
        totals[5] = m->st[0] = m->st[1] = VBM_OGG_DEMUX_ECAP;
        return VBM_OK;
    }
    for (long long i = 0; i < ncand; i++) oggrs_judge(T, m->pow, data, m->off[m->cand[i].file + 1], m->cand[i]);
    long long pages = 0, entries = 0;
    for (int f = 0; f < nfiles; f++) {
        const long long lo = oggrs_lower_bound(m->cand, ncand, m->off[f]), hi = oggrs_lower_bound(m->cand, ncand, m->off[f + 1]);
        oggrs_resolve_file(m->cand + lo, hi - lo, m->off[f], m->off[f + 1], m->pages + lo, m->side + lo, m->ent + lo,
                           m->npages[f], m->nent[f], events[f]);
        m->cand_lo[f] = lo;
        m->page_base[f] = pages;
        m->file_links[f] = file_links[f] = entries;
        pages += m->npages[f];
        entries += m->nent[f];
    }
    m->page_base[nfiles] = pages;
    m->file_links[nfiles] = file_links[nfiles] = entries;
    const bool fits = entries <= entry_cap;
    long long packets = 0, payload = 0, header = 0;
    for (int f = 0; f < nfiles; f++)
        for (long long k = 0; k < m->nent[f]; k++) {
            vbm_ogg_file_info fi = m->ent[m->cand_lo[f] + k];
            fi.packet_base = packets, fi.payload_base = payload, fi.header_base = header;
            packets += fi.packets;
            payload += fi.payload_bytes;
            header += (long long)fi.header_bytes[0] + fi.header_bytes[1] + fi.header_bytes[2];
            m->info[m->file_links[f] + k] = fi;
            if (fits) info[m->file_links[f] + k] = fi;
        }
    m->ctl[CTL_ENTRIES] = totals[0] = entries;
    m->ctl[CTL_PACKETS] = totals[1] = packets;
    m->ctl[CTL_PAYLOAD] = totals[2] = payload;
    m->ctl[CTL_HEADER] = totals[3] = header;
    totals[4] = ncand;
    totals[5] = m->st[0] = m->st[1] = fits ? 0 : VBM_OGG_DEMUX_ECAP;
    return VBM_OK;
}

extern "C" int vbm_host_ogg_resync_fill(vbm_ogg_resync *m, uint8_t *headers, long long header_cap, uint8_t *payload,
                                        long long payload_cap, long long *offsets, long long *granulepos, uint8_t *eos,
                                        uint8_t *gap, long long packet_cap)
{
    int rc = check_fill(m, true, headers, header_cap, payload, payload_cap, offsets, granulepos, eos, gap, packet_cap,
                        "vbm_host_ogg_resync_fill");
    if (rc) return rc;
    if (m->st[0] || m->ctl[CTL_PACKETS] > packet_cap || m->ctl[CTL_PAYLOAD] > payload_cap || m->ctl[CTL_HEADER] > header_cap) {
        m->st[1] = VBM_OGG_DEMUX_ECAP;
        return VBM_OK;
    }
    m->st[1] = 0;
    const OggDmxOut out = {headers, payload, offsets, granulepos, eos};
    offsets[0] = 0;
    for (int f = 0; f < m->nfiles; f++)
        for (long long k = 0; k < m->npages[f]; k++) {
            const long long slot = m->cand_lo[f] + k;
            const OggRsSide &sd = m->side[slot];
            OggDmxPageCtx c;
            oggrs_page_ctx(m->data, m->pages[slot], sd, m->info[m->file_links[f] + sd.entry], c);
            oggdmx_page_packet_ends(c, out);
            long long g0, g1;
            oggrs_gap_range(c, sd, g0, g1);
            for (long long q = g0; q < g1; q++) gap[c.packet_base + q] = q == sd.gap_pkt ? 1 : 0;
            const OggDmxSplit s = oggrs_body_split(c, sd, out);
            if (s.n_h) memcpy(s.dst_h, s.src_h, (size_t)s.n_h);
            if (s.n_p) memcpy(s.dst_p, s.src_p, (size_t)s.n_p);
        }
    return VBM_OK;
}
