// Ogg demux for many whole files at once: the acceptance rules of demux() in capi_stream.cpp (vbm_ogg_demux), written
// once for the host twin (vbm_host_ogg_demux_*) and the device kernels (ogg_demux.hip).  Page format: the reference's
// doc/framing.html.  The incremental form (ogg_feed.h, ogg_feed.hip) uses the same statements: the page walk and the
// counts it carries, the CRC, a page's fields, the packet-end rule, the body split, and the device helpers at the end.
//
// What makes the rule parallel: demux() appends the body of every page to one byte run per file and cuts it where a
// lacing value below 255 ends a packet.  So a body byte's place in the output is the number of body bytes in front of
// it in its file, and a packet's end is the body byte count through the segment that ends it.  With H = the end of
// the third packet and E = the end of the last completed packet, bytes [0, H) are the header packets, [H, E) the audio
// payload, and anything from E on is the unterminated packet that is dropped.  A page needs to know only the body bytes
// and completed packets in front of it (OggDmxPage); the walk that finds them is the serial part, one lane per file.
//
// Workspace, sized at create from max_files / max_bytes: a page is at least 27 bytes, so file f (bytes
// [off[f], off[f+1]) of the call's data) has at most (off[f+1] - off[f]) / 27 pages, and its records start at slot
// (off[f] - off[0]) / 27: sums of floors stay below the floor of the sum, so files never share a slot and no scan is
// needed before the walk.  That is max_bytes / 27 + 1 records of 32 B, about 1.2 bytes per input byte.  The pages that
// were found are then numbered densely through an exclusive scan of the files' page counts (page_base), and the
// page-parallel kernels map a dense number back to file and slot by a binary search in it.
#pragma once
#include <stdint.h>

#include "ogg_mux.h"

struct OggDmxPage {          // one page the walk accepted
    long long at;            // first byte of the page in the call's data
    long long body_before;   // body bytes of the file's pages in front of it
    long long pkt_before;    // packets completed in front of it
    int len;                 // 27 + nseg + body bytes
    int pad;
};

struct OggDmxCounts {       // what a walk carries from page to page, and the feed from call to call; all zero = no page yet
    long long body, packets; // body bytes seen, packets completed
    long long last_end;      // body bytes through the last completed packet
    long long h0, h1, h2;    // ... through each of the first three packets
    uint32_t serial, seq;    // the stream's serial number (once a page has been seen), the next page number
};

struct OggDmxWalk {          // one file while its pages are walked
    long long pos, end;      // next byte to read, end of the file
    OggDmxCounts cnt;
    int partial;             // a packet is open at the end of the last page
};

VBMX_HD uint32_t oggdmx_rd32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

VBMX_HD long long oggdmx_rd64(const uint8_t *p)
{
    return (long long)((unsigned long long)oggdmx_rd32(p) | ((unsigned long long)oggdmx_rd32(p + 4) << 32));
}

VBMX_HD void oggdmx_walk_begin(OggDmxWalk &w, long long begin, long long end)
{
    w.pos = begin, w.end = end;
    w.cnt = OggDmxCounts{};
    w.partial = 0;
}

// Segments [from, nseg) of the page at h laid onto the counts: a lacing value below 255 ends a packet.
VBMX_HD void oggdmx_lacing(const uint8_t *h, int from, int nseg, OggDmxCounts &c, int &partial)
{
    for (int i = from; i < nseg; i++) {
        const int lv = h[27 + i];
        c.body += lv;
        partial = lv == 255;
        if (lv < 255) {
            if (c.packets == 0) c.h0 = c.body;
            if (c.packets == 1) c.h1 = c.body;
            if (c.packets == 2) c.h2 = c.body;
            c.packets++;
            c.last_end = c.body;
        }
    }
}

// The next page of the file, and the only reader of a page header:
//    1  the page is taken: its record is in pg, and w has moved past it (by at least 27 bytes)
//    0  w.pos has reached w.end
//   -1  the header breaks a rule of demux() (CRC apart, which the page-parallel pass checks)
//   -2  the header, the lacing table or the body is not all in front of w.end
// A header that is all there is judged before the rest of the page is looked for, so a caller that may see more bytes
// later (the feed) treats -2 as "not yet"; for a whole file both are failures.  No byte is read before it is known to
// lie in front of w.end, and w is untouched unless the result is 1.
VBMX_HD int oggdmx_walk_step(const uint8_t *data, OggDmxWalk &w, OggDmxPage &pg)
{
    if (w.pos >= w.end) return 0;
    const long long left = w.end - w.pos;
    if (left < 27) return -2;                                      // truncated page header
    const uint8_t *h = data + w.pos;
    if (h[0] != 'O' || h[1] != 'g' || h[2] != 'g' || h[3] != 'S') return -1;
    if (h[4] != 0) return -1;                                      // stream structure version
    const int flags = h[5], nseg = h[26];
    if (!(flags & 1) && w.partial) return -1;                      // a packet continues into a page that is not a continuation
    const uint32_t sno = oggdmx_rd32(h + 14), seq = oggdmx_rd32(h + 18);
    if (w.cnt.seq != 0 && sno != w.cnt.serial) return -1;          // chained or multiplexed streams
    if (seq != w.cnt.seq) return -1;                               // page sequence counts from 0
    if (left - 27 < nseg) return -2;                               // truncated lacing table
    OggDmxCounts c = w.cnt;
    int partial = w.partial;
    oggdmx_lacing(h, 0, nseg, c, partial);
    const long long body_len = c.body - w.cnt.body;
    if (left - 27 - nseg < body_len) return -2;                    // truncated body
    pg.at = w.pos;
    pg.body_before = w.cnt.body;
    pg.pkt_before = w.cnt.packets;
    pg.len = 27 + nseg + (int)body_len;
    pg.pad = 0;
    c.serial = sno;
    c.seq = seq + 1;                                               // 2^32 pages would need a file of 108 GB
    w.cnt = c;
    w.partial = partial;
    w.pos += pg.len;
    return 1;
}

// what the walk leaves in a file's info: counts of a good file, VBM_EOGG and zeros otherwise (bases: the scan)
VBMX_HD void oggdmx_walk_end(const OggDmxWalk &w, bool ok, int npages, vbm_ogg_file_info &fi)
{
    const OggDmxCounts &c = w.cnt;
    ok = ok && c.packets >= 3;                                     // fewer than three header packets
    ok = ok && c.h2 < (1ll << 31);                                 // header_bytes are ints: no Vorbis header comes near
    fi.status = ok ? 0 : VBM_EOGG;
    fi.pages = ok ? npages : 0;
    fi.serialno = ok ? c.serial : 0u;
    fi.header_bytes[0] = ok ? (int)c.h0 : 0;
    fi.header_bytes[1] = ok ? (int)(c.h1 - c.h0) : 0;
    fi.header_bytes[2] = ok ? (int)(c.h2 - c.h1) : 0;
    fi.packets = ok ? c.packets - 3 : 0;
    fi.payload_bytes = ok ? c.last_end - c.h2 : 0;
    fi.packet_base = fi.payload_base = fi.header_base = 0;
}

VBMX_HD void oggdmx_fail_file(vbm_ogg_file_info &fi)
{
    fi.status = VBM_EOGG;
    fi.pages = 0;
    fi.serialno = 0;
    fi.header_bytes[0] = fi.header_bytes[1] = fi.header_bytes[2] = 0;
    fi.packets = fi.payload_bytes = 0;
}

// ---- CRC of a page: the code of ogg_mux.h over any byte run, combined by its linearity ------------------------------
// T: the 256 entries of oggmux_crc_entry
VBMX_HD uint32_t oggdmx_crc_run(const uint32_t *T, uint32_t crc, const uint8_t *p, int n)
{
    int i = 0;
    for (; i < n && ((uintptr_t)(p + i) & 3); i++) crc = (crc << 8) ^ T[((crc >> 24) ^ p[i]) & 0xff];
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = *(const uint32_t *)(p + i);
        crc = (crc << 8) ^ T[((crc >> 24) ^ w) & 0xff];
        crc = (crc << 8) ^ T[((crc >> 24) ^ (w >> 8)) & 0xff];
        crc = (crc << 8) ^ T[((crc >> 24) ^ (w >> 16)) & 0xff];
        crc = (crc << 8) ^ T[((crc >> 24) ^ (w >> 24)) & 0xff];
    }
    for (; i < n; i++) crc = (crc << 8) ^ T[((crc >> 24) ^ p[i]) & 0xff];
    return crc;
}

// The CRC field counts as zero while the page is summed.  The code is linear, so the sum over the page as it stands
// differs from that by the code of the four field bytes alone, moved to their place: len - 26 bytes follow them.
// whole = the code of all len bytes of the page at h; true when the field holds the page's checksum.
VBMX_HD bool oggdmx_crc_matches(const uint32_t *T, const OggMuxPow &pw, const uint8_t *h, int len, uint32_t whole)
{
    uint32_t field = 0;
    for (int i = 22; i < 26; i++) field = (field << 8) ^ T[((field >> 24) ^ h[i]) & 0xff];
    return (whole ^ oggmux_crc_shift(pw, field, (uint32_t)(len - 26))) == oggdmx_rd32(h + 22);
}

// the serial form: the page at h, len bytes, carries its own checksum
VBMX_HD bool oggdmx_page_crc_ok(const uint32_t *T, const OggMuxPow &pw, const uint8_t *h, int len)
{
    return oggdmx_crc_matches(T, pw, h, len, oggdmx_crc_run(T, 0, h, len));
}

// ---- fill: where a page's segments and body bytes go ---------------------------------------------------------------
struct OggDmxOut {           // the buffers of a fill call
    uint8_t *headers, *payload;
    long long *offsets, *granulepos;
    uint8_t *eos;
};

struct OggDmxPageCtx {       // a page of a good file, as fill sees it
    const uint8_t *h;        // the page
    int nseg, flags, body_len;
    long long granule, body_before, pkt_before;
    long long H, E;          // end of the header packets, end of the last completed packet (body bytes of the file)
    long long packet_base, payload_base, header_base;
};

// what a page record and the page's own header say of it; pkt_before, H, E and the bases are the caller's
VBMX_HD void oggdmx_page_fields(const uint8_t *data, const OggDmxPage &pg, OggDmxPageCtx &c)
{
    c.h = data + pg.at;
    c.nseg = c.h[26];
    c.flags = c.h[5];
    c.body_len = pg.len - 27 - c.nseg;
    c.granule = oggdmx_rd64(c.h + 6);
    c.body_before = pg.body_before;
}

VBMX_HD void oggdmx_page_ctx(const uint8_t *data, const OggDmxPage &pg, const vbm_ogg_file_info &fi, OggDmxPageCtx &c)
{
    oggdmx_page_fields(data, pg, c);
    c.pkt_before = pg.pkt_before;
    c.H = (long long)fi.header_bytes[0] + fi.header_bytes[1] + fi.header_bytes[2];
    c.E = c.H + fi.payload_bytes;
    c.packet_base = fi.packet_base, c.payload_base = fi.payload_base, c.header_base = fi.header_base;
}

// A segment that ends a packet (lacing value below 255): `ends_before` packets end on the page in front of it,
// `bytes_through` body bytes of the page lie up to its end, `last` when no later segment of the page ends a packet.
// Packet q of the file ends here.  Audio packet k = q - 3 gets its end offset, granule position and eos; the end of
// the third header packet is the start of audio packet 0, offsets[packet_base] = payload_base.
VBMX_HD void oggdmx_packet_end(const OggDmxPageCtx &c, const OggDmxOut &o, int ends_before, int bytes_through, bool last)
{
    const long long q = c.pkt_before + ends_before;
    if (q < 2) return;
    o.offsets[c.packet_base + (q - 2)] = c.payload_base + (c.body_before + bytes_through - c.H);
    if (q < 3) return;
    o.granulepos[c.packet_base + (q - 3)] = last ? c.granule : -1;
    o.eos[c.packet_base + (q - 3)] = ((c.flags & 4) && last) ? 1 : 0;
}

// every packet end of a page, segment after segment (the host fills; the kernels: dmx_wave_packet_ends)
VBMX_HD void oggdmx_page_packet_ends(const OggDmxPageCtx &c, const OggDmxOut &o)
{
    int last_end = -1, bytes = 0, ends = 0;
    for (int i = 0; i < c.nseg; i++)
        if (c.h[27 + i] < 255) last_end = i;
    for (int i = 0; i < c.nseg; i++) {
        bytes += c.h[27 + i];
        if (c.h[27 + i] < 255) oggdmx_packet_end(c, o, ends++, bytes, i == last_end);
    }
}

// The page's body is bytes [body_before, body_before + body_len) of the file's run: the part below H goes to the
// headers, the part in [H, E) to the payload.  Either may be empty, and the cut may fall anywhere in the body.
struct OggDmxSplit {
    const uint8_t *src_h, *src_p;
    uint8_t *dst_h, *dst_p;
    long long n_h, n_p;
};

VBMX_HD OggDmxSplit oggdmx_body_split(const OggDmxPageCtx &c, const OggDmxOut &o)
{
    const uint8_t *body = c.h + 27 + c.nseg;
    const long long a = c.body_before, b = c.body_before + c.body_len;
    const long long he = b < c.H ? b : c.H;                        // [a, he) headers
    const long long pa = a > c.H ? a : c.H, pe = b < c.E ? b : c.E;   // [pa, pe) payload
    OggDmxSplit s;
    s.n_h = he > a ? he - a : 0;
    s.src_h = body;
    s.dst_h = o.headers + c.header_base + a;
    s.n_p = pe > pa ? pe - pa : 0;
    s.src_p = body + (pa - a);
    s.dst_p = o.payload + c.payload_base + (pa - c.H);
    return s;
}

// dense page number -> file: the last f with page_base[f] <= p (page_base[nfiles] = pages in all, p below it)
VBMX_HD int oggdmx_file_of_page(const long long *page_base, int nfiles, long long p)
{
    int lo = 0, hi = nfiles - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (page_base[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ... and its number among that file's (list entry's) pages
VBMX_HD int oggdmx_entry_of_page(const long long *page_base, int n, long long p, long long &k)
{
    const int i = oggdmx_file_of_page(page_base, n, p);
    k = p - page_base[i];
    return i;
}

VBMX_HD long long oggdmx_first_slot(const long long *off, int f) { return (off[f] - off[0]) / 27; }

#ifdef __HIPCC__
// ---- device helpers of the single-block scans and the page-parallel kernels (ogg_demux.hip, ogg_feed.hip) -------------
// exclusive prefix of v over the block's 256 threads on top of `carry`, which moves on by the block's sum
__device__ __forceinline__ long long block_exclusive(long long v, long long &carry, long long *wave_sum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long x = v;
    for (int dist = 1; dist < 64; dist <<= 1) {
        const long long y = __shfl_up(x, dist, 64);
        if (lane >= dist) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    long long at = carry + x - v, total = 0;
    for (int k = 0; k < 4; k++) {
        if (k < wave) at += wave_sum[k];
        total += wave_sum[k];
    }
    carry += total;
    __syncthreads();                                // wave_sum is rewritten by the next scan
    return at;
}

// exclusive prefix over v[0, n) by one block of 256 threads, four consecutive entries per thread and step -> out, *total
template <int STRIDE>
__device__ __forceinline__ void block_scan_array(int n, const long long *v, long long *out, long long *total, long long *wave_sum)
{
    long long carry = 0;
    for (int first = 0; first < n; first += 1024) {
        const int i0 = first + threadIdx.x * 4;
        long long x[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            x[j] = i0 + j < n ? v[(long long)(i0 + j) * STRIDE] : 0;
            sum += x[j];
        }
        long long at = block_exclusive(sum, carry, wave_sum);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i0 + j < n) out[(long long)(i0 + j) * STRIDE] = at;
            at += x[j];
        }
    }
    if (threadIdx.x == 0) *total = carry;
}

// up to four bytes at p, the first `avail` of which lie in front of the run's end (avail may be negative) -> one
// word, the first byte lowest; what is not there reads as 0
__device__ __forceinline__ uint32_t dmx_load4(const uint8_t *p, long long avail)
{
    uint32_t w = 0;
    if (avail >= 4) {
        __builtin_memcpy(&w, p, 4);
    } else {
        for (int j = 0; j < 3; j++)
            if (j < avail) w |= (uint32_t)p[j] << (8 * j);
    }
    return w;
}

// The CRC of the page at h, len bytes, by the 64 lanes of a wavefront: lane l takes bytes [l * chunk, (l + 1) * chunk),
// multiplies by x^(8 * bytes after it), and the xor over the lanes is the code of the page as it stands.  True (in every
// lane) when the field holds the page's checksum.
__device__ __forceinline__ bool dmx_wave_page_crc(const uint32_t *T, const OggMuxPow &pw, const uint8_t *h, int len, int lane)
{
    const int chunk = (len + 63) >> 6, a = lane * chunk, b = min(len, a + chunk);
    uint32_t crc = 0;
    if (a < b) crc = oggmux_crc_shift(pw, oggdmx_crc_run(T, 0, h + a, b - a), (uint32_t)(len - b));
    for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
    return oggdmx_crc_matches(T, pw, h, len, crc);
}

// n bytes src -> dst by the 64 lanes of a wavefront.  Dword stores to the aligned middle of dst; a misaligned source is
// read as aligned dwords that may begin up to three bytes in front of src (the page's lacing table lies there) and never
// reach past src + n: the file may end with this body.
__device__ __forceinline__ void dmx_wave_copy(uint8_t *dst, const uint8_t *src, int n, int lane)
{
    const int lead = min(n, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    if (lane < lead) dst[lane] = src[lane];
    int nd = (n - lead) >> 2;
    const uint8_t *s0 = src + lead;
    const int sh = (int)((uintptr_t)s0 & 3) * 8;
    const uint32_t *sa = (const uint32_t *)(s0 - ((uintptr_t)s0 & 3));
    uint32_t *da = (uint32_t *)(dst + lead);
    if (sh == 0) {
        for (int i = lane; i < nd; i += 64) da[i] = sa[i];
    } else {
        // dword i needs sa[i] and sa[i + 1]: both must end at or before src + n
        const int whole = (int)((src + n - (const uint8_t *)sa) >> 2);
        nd = max(0, min(nd, whole - 1));
        for (int i = lane; i < nd; i += 64) da[i] = (sa[i] >> sh) | (sa[i + 1] << (32 - sh));
    }
    for (int i = lead + nd * 4 + lane; i < n; i += 64) dst[i] = src[i];
}

// The packet ends of a page by the 64 lanes of a wavefront: four lacing values per lane, a wave prefix sum gives every
// packet end its CSR slot.
__device__ __forceinline__ void dmx_wave_packet_ends(const OggDmxPageCtx &c, const OggDmxOut &out, int lane)
{
    // segments 4 * lane .. 4 * lane + 3; bytes (<= 65025) and packet ends (<= 255) of a page share one word
    int lv[4], mine = 0, last_end = -1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = lane * 4 + j;
        lv[j] = i < c.nseg ? c.h[27 + i] : -1;
        if (lv[j] >= 0) mine += lv[j] + (lv[j] < 255 ? 1 << 20 : 0);
        if (lv[j] >= 0 && lv[j] < 255) last_end = i;
    }
    int x = mine;
    for (int dist = 1; dist < 64; dist <<= 1) {
        const int y = __shfl_up(x, dist, 64);
        if (lane >= dist) x += y;
    }
    for (int m = 32; m >= 1; m >>= 1) last_end = max(last_end, __shfl_xor(last_end, m, 64));
    int bytes = (x - mine) & 0xfffff, ends = (x - mine) >> 20;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (lv[j] < 0) continue;
        bytes += lv[j];
        if (lv[j] < 255) oggdmx_packet_end(c, out, ends++, bytes, lane * 4 + j == last_end);
    }
}
#endif
