// Sample windows of a range store's streams cut into Ogg Vorbis files on the device, without decoding a packet (rule,
// refusals and workspace: ogg_cut.h), the host twin, and the C ABI over both (include/vorbis_mi355x.h, "Ogg cut"; host
// scaffold: twin_host.h).  The host does the packet search of vbm_synthesis_ranges over the store's host index
// (vbm_range_find) and sends one record per range up through the stage, with the sets of header pages behind them.
//
//   k_cut_plan   one wavefront per range, run twice.  The lanes fetch offsets and index of 64 packets at a time; the page
//                walk over them is the same in every lane (oggcut_packet).  The first run leaves the range's status,
//                byte count and page count; the second, behind the scan, writes the page records where the scan put them
//   k_cut_scan   one block: exclusive scans of bytes -> d_out_offsets and of pages -> the page slots; the capacity check
//   k_cut_emit   one wavefront per page slot, slots dealt out over a fixed grid.  Slot 0 of a range: its header pages,
//                copied from the uploaded set, then the range's serial number written into each and the page's CRC
//                corrected from the old one (oggcut_reserial_crc: no second pass over the page).  Every other: header and lacing table built in LDS, the CRC in 64
//                chunks combined by the linearity of the code, the body one contiguous slice of the store's data
//                (16-byte stores, a misaligned source as two aligned loads and a shift: ogg_emit.h)
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>

#include "ogg_cut.h"
#include "ogg_demux.h"
#include "ogg_emit.h"
#include "range_plan.h"
#include "twin_host.h"

namespace {

constexpr int kEmitBlocks = 16384;      // k_cut_emit's grid: 64 wavefronts per compute unit of 256

// ---- kernels ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(64) k_cut_plan(int write, const OggCutRange *recs, const long long *offsets, long long data_bytes,
                                                 const int *begin, const int *end, const long long *out_start,
                                                 long long *bytes, long long *npages, int *status, const int *word,
                                                 const long long *page_base, OggCutPage *pages)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const OggCutRange rg = recs[r];
    if (write && (*word != 0 || rg.got == 0 || status[r] != 0)) return;
    int st = 0;
    OggCutWalk w;                                   // the same in every lane
    OggCutPage *pg = write ? pages + page_base[r] + 1 : nullptr;
    if (rg.got > 0) {
        for (int base = rg.pre; base <= rg.m && !st; base += 64) {
            const int j = base + lane;
            long long o0 = 0, o1 = 0, oe = 0;
            int bg = 0;
            if (j <= rg.m) {
                o0 = offsets[j], o1 = offsets[j + 1];
                bg = begin[j];
                oe = out_start[j] + (end[j] - bg);
            }
            const bool bad = o0 < 0 || o1 < o0 || o1 > data_bytes || o1 - o0 > (1 << 24);      // (d)
            if (__ballot(bad)) {
                st = VBM_OGG_CUT_ESHAPE;
                break;
            }
            if (base == rg.pre) oggcut_begin(w, rg, __shfl(o0, 0, 64));
            const int cnt = min(64, rg.m - base + 1);
            for (int t = 0; t < cnt && !st; t++) {
                const long long at = __shfl(o0, t, 64);
                st = oggcut_packet(w, rg, base + t, at, (int)(__shfl(o1, t, 64) - at), __shfl(oe, t, 64), __shfl(bg, t, 64), pg,
                                   write && lane == 0);
            }
        }
    }
    if (write || lane != 0) return;
    const bool out = rg.got > 0 && !st;
    bytes[r] = out ? w.bytes : 0;
    npages[r] = out ? 1 + w.npages : 0;
    status[r] = st;
}

__global__ void __launch_bounds__(256) k_cut_scan(int n, const long long *bytes, const long long *npages, long long *out_offsets,
                                                  long long *page_base, long long out_cap, long long max_pages, int *word,
                                                  int *status)
{
    __shared__ long long wave_sum[4];
    block_scan_array<1>(n, bytes, out_offsets, out_offsets + n, wave_sum);
    block_scan_array<1>(n, npages, page_base, page_base + n, wave_sum);
    if (threadIdx.x == 0) {                         // thread 0 wrote both totals itself
        const int s = out_offsets[n] > out_cap || page_base[n] > max_pages ? VBM_OGG_CUT_ECAP : 0;
        *word = s;
        status[n] = s;
    }
}

__global__ void __launch_bounds__(64) k_cut_emit(int n, OggMuxPow pw, const OggCutRange *recs, const uint8_t *hdr_pages,
                                                 const uint8_t *data, const long long *offsets, const int *word,
                                                 const long long *page_base, const OggCutPage *pages,
                                                 const long long *out_offsets, uint8_t *out, long long out_cap)
{
    if (*word != 0) return;                         // the outputs do not fit: nothing is written
    const int lane = threadIdx.x;
    __shared__ uint32_t T[256];
    __shared__ uint8_t hdr[27 + 255 + 2];
    for (int i = lane; i < 256; i += 64) T[i] = oggmux_crc_entry(i);
    __syncthreads();
    const long long total = page_base[n];
    for (long long p = blockIdx.x; p < total; p += gridDim.x) {
        const int r = oggdmx_file_of_page(page_base, n, p);
        const OggCutRange rg = recs[r];
        const long long at0 = out_offsets[r];
        if (p == page_base[r]) {                    // the header pages, as the host writer made them
            if (at0 + rg.hdr_bytes > out_cap) continue;
            const uint8_t *src = hdr_pages + rg.hdr_at;
            vec_copy<64>(out + at0, src, rg.hdr_bytes, lane);
            __syncthreads();                        // the copy's stores are done before the patch's
            // the range's serial number into every page (the host has checked that they are whole pages)
            for (int k = 0, pos = 0; k < rg.hdr_pages; k++) {
                const uint8_t *h = src + pos;
                const int nseg = h[26];
                int body = 0;
                for (int i = lane; i < nseg; i += 64) body += h[27 + i];
                for (int m = 32; m >= 1; m >>= 1) body += __shfl_xor(body, m, 64);
                const int len = 27 + nseg + body;
                const uint32_t crc = oggcut_reserial_crc(pw, oggcut_le32(h + 22), oggcut_le32(h + 14), (uint32_t)rg.serialno, (uint32_t)len);
                if (lane < 4) {
                    out[at0 + pos + 14 + lane] = (uint8_t)((uint32_t)rg.serialno >> (8 * lane));
                    out[at0 + pos + 22 + lane] = (uint8_t)(crc >> (8 * lane));
                }
                pos += len;
            }
            continue;
        }
        const OggCutPage pg = pages[p];
        const int hl = 27 + pg.nseg, L = hl + pg.body_bytes;
        __syncthreads();                            // hdr: the page before is done with it
        if (lane == 0) {
            OggMuxPage mp;
            mp.granule = pg.granule;
            mp.nseg = pg.nseg, mp.body_bytes = pg.body_bytes, mp.flags = pg.flags, mp.pageno = pg.pageno;
            mp.lace_at = mp.body_at = 0;
            oggmux_page_header(mp, rg.serialno, hdr);
        }
        // the lacing table, 64 packets at a time from pkt0 on: every lane writes its packet's values
        int pos = 0, skip = pg.skip0;
        for (int pkt = pg.pkt0; pos < pg.nseg && pkt <= rg.m; pkt += 64, skip = 0) {
            const int j = pkt + lane;
            const int bytes = j <= rg.m ? (int)(offsets[j + 1] - offsets[j]) : 0;
            const int cnt = j <= rg.m ? bytes / 255 + 1 - (lane == 0 ? skip : 0) : 0;
            int x = cnt;
            for (int dist = 1; dist < 64; dist <<= 1) {
                const int y = __shfl_up(x, dist, 64);
                if (lane >= dist) x += y;
            }
            const int first = pos + x - cnt;
            if (cnt > 0 && first < pg.nseg) {
                int last;
                const int mine = oggcut_lacing(bytes, lane == 0 ? skip : 0, pg.nseg - first, &last);
                for (int i = 0; i < mine - 1; i++) hdr[27 + first + i] = 255;
                hdr[27 + first + mine - 1] = (uint8_t)last;
            }
            pos += __shfl(x, 63, 64);
        }
        __syncthreads();

        // CRC: lane l takes bytes [l * chunk, (l + 1) * chunk) of the page
        const uint8_t *body = data + pg.body_src;
        const int chunk = (L + 63) >> 6, a = lane * chunk, b = min(L, a + chunk);
        uint32_t crc = 0;
        if (a < b) {
            int q = a;
            for (; q < b && q < hl; q++) crc = crc_byte(T, crc, hdr[q]);
            if (q < b) crc = crc_run(T, crc, body + (q - hl), b - q);
        }
        crc = crc_wave_combine(pw, crc, a < b, (uint32_t)(L - b));
        if (lane < 4) hdr[22 + lane] = (uint8_t)((crc >> (8 * lane)) & 0xff);
        __syncthreads();

        const long long at = at0 + pg.out_at;
        if (at + L > out_cap) continue;             // second line of defence: the scan has checked the total
        uint8_t *dst = out + at;
        for (int i = lane; i < hl; i += 64) dst[i] = hdr[i];
        vec_copy<64>(dst + hl, body, pg.body_bytes, lane);
    }
}

}  // namespace

// ---- host side (scaffold: twin_host.h) --------------------------------------------------------------------------

struct vbm_ogg_cutter {
    bool host = false;
    int max_ranges = 0;
    long long max_out_bytes = 0, max_header_bytes = 0, max_pages = 0;
    OggMuxPow pow;
    TwinMem mem;                         // owns the workspace
    uint8_t *args = nullptr;             // the call's OggCutRange records, then its header pages
    long long *bytes = nullptr;          // [max_ranges] output bytes, what the scan reads
    long long *npages = nullptr;         // [max_ranges] page slots
    long long *page_base = nullptr;      // [max_ranges + 1]
    OggCutPage *pages = nullptr;         // [max_pages]
    int *word = nullptr;                 // the status word of the last call
    ArgStage stage;                      // device form: args goes up through it
    std::vector<OggCutRange> recs;       // host twin
};

namespace {

struct CutIndex {                        // what the search reads, of a store or of the twin's arrays
    int S;
    const long long *first;
    const int *status;
    const long long *out_end, *totals;
    const long long *last, *lo;          // a live store's ends of streams and first retained samples, else null
};

int create(vbm_ogg_cutter **out, int max_ranges, long long max_out_bytes, long long max_header_bytes, bool host)
{
    if (!out || max_ranges < 1 || max_out_bytes < 0 || max_header_bytes < 0)
        return fail(VBM_EINVAL, "vbm_ogg_cut_create: bad argument (max_ranges >= 1, max_out_bytes >= 0, max_header_bytes >= 0)");
    if (!host) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(VBM_ENODEV, "vbm_ogg_cut_create: no HIP device");
    }
    vbm_ogg_cutter *m = new (std::nothrow) vbm_ogg_cutter();
    if (!m) return fail(VBM_EFAULT, "vbm_ogg_cut_create: out of memory");
    m->host = m->mem.host = host;
    m->max_ranges = max_ranges;
    m->max_out_bytes = max_out_bytes;
    m->max_header_bytes = max_header_bytes;
    m->max_pages = oggcut_max_pages(max_ranges, max_out_bytes);
    m->pow = oggmux_pow_table();
    const size_t R = (size_t)max_ranges, arg_bytes = R * sizeof(OggCutRange) + (size_t)max_header_bytes;
    const char *who = "vbm_ogg_cut";
    int rc = m->mem.get(m->bytes, R, who);
    if (!rc) rc = m->mem.get(m->npages, R, who);
    if (!rc) rc = m->mem.get(m->page_base, R + 1, who);
    if (!rc) rc = m->mem.get(m->pages, (size_t)m->max_pages, who);
    if (!rc) rc = m->mem.get(m->word, 1, who);
    if (!rc && !host) rc = m->mem.get(m->args, arg_bytes, who);
    if (!rc && !host) rc = m->stage.create(arg_bytes, "vbm_ogg_cut_create: staging");
    if (rc) {
        vbm_ogg_cut_destroy(m);
        return rc;
    }
    *out = m;
    return VBM_OK;
}

// The arguments checked and the search done: recs [nranges], got_starts / got_lengths.  The header pages of range r are
// set header_ids[r] (null: r) of the nheaders sets hdr[hdr_offsets[e], hdr_offsets[e + 1]), whole pages each.
int prepare(const vbm_ogg_cutter *m, bool host, const CutIndex &ix, int nranges, const int *stream_ids, const long long *starts,
            const long long *lengths, const int *serialnos, int nheaders, const uint8_t *hdr, const long long *hdr_offsets,
            const int *header_ids, const uint8_t *out, long long out_cap, const void *out_offsets, const int *status, long long *got_starts,
            long long *got_lengths, OggCutRange *recs, const char *who_)
{
    const std::string who(who_);
    if (int rc = check_kind(m, host, who_, "cut")) return rc;
    if (nranges < 0 || nranges > m->max_ranges) return fail(VBM_EINVAL, who + ": nranges is negative or above max_ranges");
    if (!out_offsets || !status || (nranges > 0 && (!stream_ids || !starts || !lengths || !got_starts || !got_lengths)))
        return fail(VBM_EINVAL, who + ": null pointer");
    if (out_cap < 0 || out_cap > m->max_out_bytes) return fail(VBM_EINVAL, who + ": out_cap is negative or above max_out_bytes");
    if (out_cap > 0 && !out) return fail(VBM_EINVAL, who + ": null output");
    if (nheaders < 0 || (nheaders > 0 && !hdr_offsets)) return fail(VBM_EINVAL, who + ": nheaders is negative, or null header_offsets");
    std::vector<int> hdr_pages((size_t)nheaders, 0);        // whole pages, counted
    if (nheaders > 0) {
        if (hdr_offsets[0] != 0) return fail(VBM_EINVAL, who + ": header_offsets[0] must be 0");
        for (int e = 0; e < nheaders; e++)
            if (hdr_offsets[e + 1] < hdr_offsets[e] || hdr_offsets[e + 1] - hdr_offsets[e] > INT_MAX)
                return fail(VBM_EINVAL, who + ": header_offsets decrease");
        if (hdr_offsets[nheaders] > m->max_header_bytes)
            return fail(VBM_EINVAL, who + ": the header pages are above max_header_bytes");
        if (hdr_offsets[nheaders] > 0 && !hdr) return fail(VBM_EINVAL, who + ": null header pages");
        for (int e = 0; e < nheaders; e++) {
            const long long bytes = hdr_offsets[e + 1] - hdr_offsets[e];
            for (long long at = 0; at < bytes; hdr_pages[e]++) {
                const uint8_t *h = hdr + hdr_offsets[e] + at;
                const long long room = bytes - at;
                long long len = room >= 27 && !memcmp(h, "OggS", 4) ? 27 + h[26] : room + 1;
                for (int k = 0; len <= room && k < h[26]; k++) len += h[27 + k];
                if (len > room) return fail(VBM_EINVAL, who + ": a set of header pages is not whole Ogg pages");
                at += len;
            }
        }
    }
    for (int r = 0; r < nranges; r++) {
        const int i = stream_ids[r];
        if (i < 0 || i >= ix.S) return fail(VBM_EINVAL, who + ": stream id out of range");
        if (starts[r] < 0 || lengths[r] < 0) return fail(VBM_EINVAL, who + ": negative start or length");
        OggCutRange &rg = recs[r];
        memset(&rg, 0, sizeof rg);
        rg.s = starts[r];
        const long long left = ix.totals[i] - rg.s;
        rg.got = left < 0 ? 0 : left < lengths[r] ? left : lengths[r];
        if (ix.lo && rg.s < ix.lo[i]) rg.got = 0;           // a live store has dropped the window's start
        rg.serialno = serialnos ? serialnos[r] : r;
        if (rg.got > 0) {
            const long long a = ix.first[i];
            if (!vbm_range_find(a, ix.last ? ix.last[i] : ix.first[i + 1], ix.status, ix.out_end, rg.s, rg.got, rg.k, rg.m, rg.pre))
                return fail(VBM_EINVAL, who + ": range store index: no pre-roll packet");
            if (rg.k == rg.m) {                             // the start cannot be trimmed as well as the end
                const long long s0 = rg.k > a ? ix.out_end[rg.k - 1] : 0;
                rg.got += rg.s - s0;
                rg.s = s0;
            }
            const int e = header_ids ? header_ids[r] : r;
            if (e < 0 || e >= nheaders) return fail(VBM_EINVAL, who + ": header id out of range");
            rg.hdr_at = hdr_offsets[e];
            rg.hdr_bytes = (int)(hdr_offsets[e + 1] - hdr_offsets[e]);
            rg.hdr_pages = hdr_pages[e];
        }
        got_starts[r] = rg.s;
        got_lengths[r] = rg.got;
    }
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_ogg_cut_create(vbm_ogg_cutter **cut, int max_ranges, long long max_out_bytes, long long max_header_bytes)
{
    return create(cut, max_ranges, max_out_bytes, max_header_bytes, false);
}

extern "C" int vbm_host_ogg_cut_create(vbm_ogg_cutter **cut, int max_ranges, long long max_out_bytes, long long max_header_bytes)
{
    return create(cut, max_ranges, max_out_bytes, max_header_bytes, true);
}

extern "C" void vbm_ogg_cut_destroy(vbm_ogg_cutter *m)
{
    if (!m) return;
    m->mem.free_all();
    m->stage.destroy();
    delete m;
}

extern "C" int vbm_ogg_cut_ranges(vbm_ogg_cutter *m, const vbm_range_store *store, int nranges, const int *stream_ids,
                                  const long long *starts, const long long *lengths, const int *serialnos, int nheaders,
                                  const uint8_t *header_pages, const long long *header_offsets, const int *header_ids,
                                  uint8_t *d_out,
                                  long long out_cap, long long *d_out_offsets, int *d_status, long long *got_starts,
                                  long long *got_lengths, void *stream)
{
    const char *who = "vbm_ogg_cut_ranges";
    if (!m || !store) return fail(VBM_EINVAL, "vbm_ogg_cut_ranges: null cutter or store");
    vbm_range_store_view v;
    vbm_range_store_get_view(store, &v);
    if (v.host) return fail(VBM_EINVAL, "vbm_ogg_cut_ranges: a host store (vbm_host_live_store_create) in a device call");
    if (v.halfrate) return fail(VBM_EINVAL, "vbm_ogg_cut_ranges: a half-rate store's positions are not packet granule positions");
    if (out_cap > 0 && d_out && v.data_bytes > 0 && (uintptr_t)d_out < (uintptr_t)(v.d_data + v.data_bytes) &&
        (uintptr_t)v.d_data < (uintptr_t)(d_out + out_cap))
        return fail(VBM_EINVAL, "vbm_ogg_cut_ranges: the output overlaps the store");
    if (m->host) return check_kind(m, false, who, "cut");
    hipStream_t q = (hipStream_t)stream;
    void *slot = nullptr;
    if (nranges > 0 && nranges <= m->max_ranges) {
        const int rc = m->stage.next(slot, "vbm_ogg_cut_ranges: hipEventSynchronize(stage)");
        if (rc) return rc;
    }
    OggCutRange *recs = (OggCutRange *)slot;
    const CutIndex ix = {v.S, v.first, v.status, v.out_end, v.totals, v.last, v.lo};
    int rc = prepare(m, false, ix, nranges, stream_ids, starts, lengths, serialnos, nheaders, header_pages, header_offsets,
                     header_ids, d_out, out_cap,
                     d_out_offsets, d_status, got_starts, got_lengths, recs, who);
    if (rc) return rc;
    // the records, and behind them the header pages, go up in one copy
    const size_t rec_bytes = (size_t)(nranges > 0 ? nranges : 0) * sizeof(OggCutRange);
    const OggCutRange *d_recs = (const OggCutRange *)m->args;
    const uint8_t *d_hdr = m->args + rec_bytes;
    if (nranges > 0) {
        const size_t hb = nheaders > 0 ? (size_t)header_offsets[nheaders] : 0;
        if (hb) memcpy((uint8_t *)slot + rec_bytes, header_pages, hb);
        rc = m->stage.send(m->args, rec_bytes + hb, q, "vbm_ogg_cut_ranges: upload");
        if (rc) return rc;
        hipLaunchKernelGGL(k_cut_plan, dim3(nranges), dim3(64), 0, q, 0, d_recs, v.d_offsets, v.data_bytes, v.d_begin, v.d_end,
                           v.d_out_start, m->bytes, m->npages, d_status, m->word, m->page_base, m->pages);
    }
    hipLaunchKernelGGL(k_cut_scan, dim3(1), dim3(256), 0, q, nranges, m->bytes, m->npages, d_out_offsets, m->page_base, out_cap,
                       m->max_pages, m->word, d_status);
    if (nranges > 0 && out_cap > 0) {
        hipLaunchKernelGGL(k_cut_plan, dim3(nranges), dim3(64), 0, q, 1, d_recs, v.d_offsets, v.data_bytes, v.d_begin, v.d_end,
                           v.d_out_start, m->bytes, m->npages, d_status, m->word, m->page_base, m->pages);
        // the page count is on the device alone: a fixed grid deals the slots out, and no more blocks than the bound
        const long long most = oggcut_max_pages(nranges, out_cap);
        hipLaunchKernelGGL(k_cut_emit, dim3((unsigned)(most < kEmitBlocks ? most : kEmitBlocks)), dim3(64), 0, q, nranges, m->pow,
                           d_recs, d_hdr, v.d_data, v.d_offsets, m->word, m->page_base, m->pages, d_out_offsets, d_out, out_cap);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_cut_ranges: launch");
}

// ---- the same on the CPU: the walk of ogg_cut.h range after range, a memcpy per page body, the table CRC --------------
extern "C" int vbm_host_ogg_cut_ranges(vbm_ogg_cutter *m, int nstreams, const long long *first, const int *status,
                                       const int *begin, const long long *out_end, const long long *totals,
                                       const uint8_t *data, const long long *offsets, long long data_bytes, int nranges,
                                       const int *stream_ids, const long long *starts, const long long *lengths,
                                       const int *serialnos, int nheaders, const uint8_t *header_pages,
                                       const long long *header_offsets, const int *header_ids, uint8_t *out, long long out_cap, long long *out_offsets, int *out_status,
                                       long long *got_starts, long long *got_lengths)
{
    const char *who = "vbm_host_ogg_cut_ranges";
    if (!m) return fail(VBM_EINVAL, "vbm_host_ogg_cut_ranges: null cutter");
    if (nstreams < 1 || !first || !totals || data_bytes < 0 || first[0] != 0 || first[nstreams] >= INT_MAX ||
        (first[nstreams] > 0 && (!status || !begin || !out_end || !offsets)) || (data_bytes > 0 && !data))
        return fail(VBM_EINVAL, "vbm_host_ogg_cut_ranges: bad index (nstreams >= 1, first[0] == 0, no null array)");
    if (out_cap > 0 && out && data_bytes > 0 && (uintptr_t)out < (uintptr_t)(data + data_bytes) &&
        (uintptr_t)data < (uintptr_t)(out + out_cap))
        return fail(VBM_EINVAL, "vbm_host_ogg_cut_ranges: the output overlaps the store");
    m->recs.resize((size_t)(nranges > 0 && nranges <= m->max_ranges ? nranges : 0));
    const CutIndex ix = {nstreams, first, status, out_end, totals, nullptr, nullptr};
    int rc = prepare(m, true, ix, nranges, stream_ids, starts, lengths, serialnos, nheaders, header_pages, header_offsets,
                     header_ids, out, out_cap,
                     out_offsets, out_status, got_starts, got_lengths, m->recs.data(), who);
    if (rc) return rc;
    // a range's walk: counts, and with `pg` its page records
    auto walk = [&](const OggCutRange &rg, OggCutWalk &w, OggCutPage *pg) {
        for (int j = rg.pre; j <= rg.m; j++) {
            const long long o0 = offsets[j], o1 = offsets[j + 1];
            if (o0 < 0 || o1 < o0 || o1 > data_bytes || o1 - o0 > (1 << 24)) return (int)VBM_OGG_CUT_ESHAPE;
            if (j == rg.pre) oggcut_begin(w, rg, o0);
            if (int st = oggcut_packet(w, rg, j, o0, (int)(o1 - o0), out_end[j], begin[j], pg, pg != nullptr)) return st;
        }
        return 0;
    };
    long long total = 0, slots = 0;
    for (int r = 0; r < nranges; r++) {
        const OggCutRange &rg = m->recs[r];
        OggCutWalk w;
        const int st = rg.got > 0 ? walk(rg, w, nullptr) : 0;
        const bool has = rg.got > 0 && !st;
        out_status[r] = st;
        if (st) got_lengths[r] = 0;                         // the twin knows: a refused range holds nothing
        out_offsets[r] = total;
        m->page_base[r] = slots;
        m->npages[r] = has ? 1 + w.npages : 0;
        total += has ? w.bytes : 0;
        slots += m->npages[r];
    }
    out_offsets[nranges] = total;
    *m->word = out_status[nranges] = total > out_cap || slots > m->max_pages ? VBM_OGG_CUT_ECAP : 0;
    if (*m->word || out_cap == 0) return VBM_OK;
    const CrcTable &T = crc_table();
    for (int r = 0; r < nranges; r++) {
        const OggCutRange &rg = m->recs[r];
        if (m->npages[r] == 0) continue;
        OggCutPage *pg = m->pages + m->page_base[r] + 1;
        OggCutWalk w;
        walk(rg, w, pg);
        uint8_t *o0 = out + out_offsets[r];
        if (rg.hdr_bytes) memcpy(o0, header_pages + rg.hdr_at, (size_t)rg.hdr_bytes);
        for (int k = 0, pos = 0; k < rg.hdr_pages; k++) {   // the range's serial number into every header page
            uint8_t *h = o0 + pos;
            int len = 27 + h[26];
            for (int i = 0; i < h[26]; i++) len += h[27 + i];
            const uint32_t crc = oggcut_reserial_crc(m->pow, oggcut_le32(h + 22), oggcut_le32(h + 14), (uint32_t)rg.serialno, (uint32_t)len);
            for (int i = 0; i < 4; i++) h[14 + i] = (uint8_t)((uint32_t)rg.serialno >> (8 * i)), h[22 + i] = (uint8_t)(crc >> (8 * i));
            pos += len;
        }
        for (int p = 0; p < w.npages; p++) {
            uint8_t *o = o0 + pg[p].out_at;
            OggMuxPage mp;
            mp.granule = pg[p].granule;
            mp.nseg = pg[p].nseg, mp.body_bytes = pg[p].body_bytes, mp.flags = pg[p].flags, mp.pageno = pg[p].pageno;
            mp.lace_at = mp.body_at = 0;
            oggmux_page_header(mp, rg.serialno, o);
            for (int pos = 0, j = pg[p].pkt0, skip = pg[p].skip0; pos < mp.nseg; j++, skip = 0) {
                int last;
                const int mine = oggcut_lacing((int)(offsets[j + 1] - offsets[j]), skip, mp.nseg - pos, &last);
                memset(o + 27 + pos, 255, (size_t)mine - 1);
                o[27 + pos + mine - 1] = (uint8_t)last;
                pos += mine;
            }
            if (mp.body_bytes) memcpy(o + 27 + mp.nseg, data + pg[p].body_src, (size_t)mp.body_bytes);
            const long long L = 27 + mp.nseg + mp.body_bytes;
            uint32_t crc = 0;
            for (long long i = 0; i < L; i++) crc = (crc << 8) ^ T.t[((crc >> 24) & 0xff) ^ o[i]];
            for (int i = 0; i < 4; i++) o[22 + i] = (uint8_t)((crc >> (8 * i)) & 0xff);
        }
    }
    return VBM_OK;
}
