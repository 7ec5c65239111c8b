// Ogg paging for many streams at once: the rule of vbm_ogg_stream_packetin / _pageout (capi_stream.cpp), written
// once for the host twin (vbm_host_ogg_mux_packets) and the device kernels (ogg_mux.hip) over a fixed-size
// per-stream state.  Page format: the reference's doc/framing.html.
//
// The rule (libogg 1.3's policy, as the host writer has it):
//   - after each packet is queued, pages go out while one is due;
//   - a page is due at the first segment in front of which lie more than 4096 body bytes and at least four
//     completed packets, the segment before it ending a packet; and at 255 segments;
//   - everything queued goes out once e_o_s has been queued, or on an explicit flush;
//   - a page's granule position is that of the last packet that ends on it, -1 if none does;
//   - the continued flag follows a page whose last lacing value was 255;
//   - e_o_s is set only on the page that empties the queue.
// Header pages are not made here: a started stream is "first page gone, page number = header pages written, queue
// empty" (vbm_ogg_mux_start_streams builds the header pages with the host writer).
//
// One call sees, per stream, the queue it carried in plus the call's packets in packetno order as ONE sequence of
// lacing values (`lacing`, `gran`: the queue's at the front, the new packets' appended) and one virtual body (the
// queued bytes, then packet after packet).  Pages take prefixes of both; nothing is erased while the rule runs
// (a head index moves), so that a packet that cannot be taken is rolled back by restoring a few scalars.  After the
// pages are written, the rest of both sequences is moved to the front and is the queue the next call starts with.
//
// Sizes, with M = max_packet_bytes, R = max_rows_per_stream:
//   queue after a drain   <= 254 segments (255 would have gone out), and no page is due on it: at every packet boundary
//                         with four or more packets in front there are at most 4096 bytes in front.  So it holds at
//                         most four packets, or at most 4096 bytes followed by one more packet:
//                             Q = min(254 * 255, max(4 * M, 4096 + M))  body bytes,
//                         which is the default queue capacity (M = 4096, stereo: 16 KiB per stream, 256 MiB at 16384
//                         streams; libogg's own bound for an unknown M, 254 * 255 + M = 69 KB per stream, would be
//                         1.1 GB).  A smaller capacity may be asked for at create: a packet after whose drain more
//                         would stay queued is refused with VBM_MUX_EQUEUE and the stream stops producing.
//   lacing values in a call <= 254 + R * (M / 255 + 1)                              (lace_cap; 526 for M = 4096, R = 16)
//   pages of a stream in a call: every page but one either carries 255 segments or more than 4096 bytes, the one is the
//                         page that empties the queue at e_o_s or on flush (a stream meets e_o_s at most once per call:
//                         rows after it are refused):
//                             P = 2 + lace_cap / 255 + (Q + R * M) / 4097               (max_pages)
// State per stream: 32 B head + lace_cap * 9 B + Q + R * 4 B rows + P * 32 B page records + 48 B call record:
// about 22 KB at M = 4096, R = 16, i.e. 360 MB at 16384 streams, of which 256 MiB are the body queues.
//
// Output bound of a call with n rows over S streams (n counted up to S * R: rows over the cap are not taken):
//   body bytes  <= S * min(Q, queue_bytes) + n * M          every queued byte and every byte of the call goes out at most once
//   segments    <= S * 254 + n * (M / 255 + 1)              likewise, one lacing byte per segment
//   pages       <= S + segments / 255 + body / 4097         per stream one emptying page; every other page consumes
//                                                           255 segments or more than 4096 bytes of its own
//   bytes       <= body + segments + 27 * pages             = vbm_ogg_mux_out_bound
#pragma once
#include <stdint.h>

#include "vorbis_mi355x.h"

#ifdef __HIPCC__
#define VBMX_HD __host__ __device__ inline
#else
#define VBMX_HD inline
#endif

enum {
    OGGMUX_PREV_OPEN = 1,   // the last page ended inside a packet
    OGGMUX_EOS = 2,         // e_o_s has been queued
    OGGMUX_STARTED = 4,     // header pages written (vbm_ogg_mux_start_streams)
    OGGMUX_FAIL_SHIFT = 8,  // sticky status of a stream that lost data (VBM_MUX_EROWS, _EQUEUE, _EPACKET) << 8
};

struct OggMuxDims {
    int nstreams, max_packet_bytes, max_rows, queue_bytes, lace_cap, max_pages;
};

struct OggMuxHead {   // carried from call to call
    int serialno, pageno, flags, nseg, nbody, pad[3];
};

struct OggMuxPage {   // one page a call writes
    long long granule;
    int nseg, body_bytes, flags, pageno;
    int lace_at;      // first lacing value, index into the call's lacing sequence
    int body_at;      // first body byte, offset into the call's virtual body
};

struct OggMuxCall {   // what the plan leaves for emit and commit
    long long out_bytes;
    int nbody_old;    // queued bytes carried in
    int body_used;    // virtual body bytes the pages take
    int body_total;   // virtual body: queue + packets taken
    int lace_used, lace_total;
    int npages, nrows;   // rows taken (a prefix of the sorted list)
    int pad[3];
};

VBMX_HD long long oggmux_q_rule(int M)
{
    long long a = 4ll * M, b = 4096ll + M;
    long long q = a > b ? a : b;
    return q < 254 * 255 ? q : 254 * 255;
}

VBMX_HD OggMuxDims oggmux_dims(int nstreams, int max_packet_bytes, int max_rows, int queue_bytes)
{
    OggMuxDims d;
    d.nstreams = nstreams;
    d.max_packet_bytes = max_packet_bytes;
    d.max_rows = max_rows;
    const long long q = oggmux_q_rule(max_packet_bytes);
    d.queue_bytes = (queue_bytes > 0 && queue_bytes < q) ? queue_bytes : (int)q;
    d.lace_cap = 254 + max_rows * (max_packet_bytes / 255 + 1);
    d.max_pages = 2 + d.lace_cap / 255 + (int)((q + (long long)max_rows * max_packet_bytes) / 4097);
    return d;
}

VBMX_HD long long oggmux_out_bound(const OggMuxDims &d, long long nrows)
{
    const long long S = d.nstreams, cap = S * d.max_rows, n = nrows < cap ? nrows : cap;
    const long long body = S * d.queue_bytes + n * d.max_packet_bytes;
    const long long segs = S * 254 + n * (d.max_packet_bytes / 255 + 1);
    const long long pages = S + segs / 255 + body / 4097;
    return body + segs + 27 * pages;
}

// vbm_ogg_stream_pageout over lacing[head, tail): 1 and the page's record when one goes out
VBMX_HD int oggmux_pageout(OggMuxHead &h, const uint8_t *lacing, const long long *gran, int &head, int tail,
                           int &body_head, int flush, OggMuxPage &pg)
{
    const int avail = tail - head, maxvals = avail > 255 ? 255 : avail;
    if (maxvals == 0) return 0;
    bool force = flush != 0 || (h.flags & OGGMUX_EOS);
    long long granule_pos = -1;
    int acc = 0, packets_done = 0, packet_just_done = 0, vals;
    for (vals = 0; vals < maxvals; vals++) {
        if (acc > 4096 && packet_just_done >= 4) { force = true; break; }
        const int lv = lacing[head + vals];
        acc += lv;
        if (lv < 255) {
            granule_pos = gran[head + vals];
            packet_just_done = ++packets_done;
        } else {
            packet_just_done = 0;
        }
    }
    if (vals == 255) force = true;
    if (!force) return 0;
    pg.granule = granule_pos;
    pg.nseg = vals;
    pg.body_bytes = acc;
    pg.flags = ((h.flags & OGGMUX_PREV_OPEN) ? 0x01 : 0) | (((h.flags & OGGMUX_EOS) && vals == avail) ? 0x04 : 0);
    pg.pageno = h.pageno;
    pg.lace_at = head;
    pg.body_at = body_head;
    head += vals;
    body_head += acc;
    h.pageno++;
    h.flags = (h.flags & ~OGGMUX_PREV_OPEN) | (lacing[head - 1] == 255 ? OGGMUX_PREV_OPEN : 0);
    return 1;
}

// One stream, one call: its rows (indices into the call's arrays, `count` of them appended in any order) are sorted
// by packetno, queued one after the other and paged by the rule.  Writes the page records and the call record, moves
// the head's page number and flags on; lacing / gran keep the whole sequence of the call (commit moves the rest down).
// Returns the stream's status.
VBMX_HD int oggmux_plan_stream(const OggMuxDims &d, OggMuxHead &h, uint8_t *lacing, long long *gran, int *rows,
                               int count, const int *packet_bytes, const vbm_packet_info *info, int flush,
                               OggMuxPage *pages, OggMuxCall &c)
{
    int status = h.flags >> OGGMUX_FAIL_SHIFT;      // a stream that lost data stays refused until it is restarted
    int n = count;
    if (n > d.max_rows) {
        n = d.max_rows;                             // which rows made it into the list is arbitrary: take none
        if (!status) status = VBM_MUX_EROWS;
    }
    for (int i = 1; i < n; i++) {                   // insertion sort: nothing depends on the order of the appends
        const int r = rows[i];
        const long long key = info[r].packetno;
        int j = i;
        for (; j > 0 && (info[rows[j - 1]].packetno > key || (info[rows[j - 1]].packetno == key && rows[j - 1] > r)); j--)
            rows[j] = rows[j - 1];
        rows[j] = r;
    }
    int head = 0, tail = h.nseg, body_head = 0, body_total = h.nbody, npages = 0, taken = 0;
    long long out_bytes = 0;
    c.nbody_old = h.nbody;
    for (int i = 0; i < n && !status; i++) {
        const int r = rows[i], bytes = packet_bytes[r];
        if (!(h.flags & OGGMUX_STARTED) || (h.flags & OGGMUX_EOS)) { status = VBM_MUX_ESTATE; break; }
        if (bytes > d.max_packet_bytes) { status = VBM_MUX_EPACKET; break; }
        const int segs = bytes / 255 + 1;
        // what a refused packet must leave as it was
        const OggMuxHead h0 = h;
        const int head0 = head, tail0 = tail, body_head0 = body_head, npages0 = npages;
        const long long out0 = out_bytes;
        for (int k = 0; k < segs - 1; k++) {
            lacing[tail] = 255;
            gran[tail++] = -1;
        }
        lacing[tail] = (uint8_t)(bytes % 255);
        gran[tail++] = info[r].granulepos;
        if (info[r].eos) h.flags |= OGGMUX_EOS;
        body_total += bytes;
        bool fits = true;
        while (fits) {
            OggMuxPage pg;
            if (!oggmux_pageout(h, lacing, gran, head, tail, body_head, 0, pg)) break;
            if (npages >= d.max_pages) { fits = false; break; }
            pages[npages++] = pg;
            out_bytes += 27 + pg.nseg + pg.body_bytes;
        }
        if (!fits || body_total - body_head > d.queue_bytes) {
            h = h0;
            head = head0, tail = tail0, body_head = body_head0, npages = npages0, out_bytes = out0;
            body_total -= bytes;
            status = VBM_MUX_EQUEUE;
            break;
        }
        taken++;
    }
    if (status == VBM_MUX_EROWS || status == VBM_MUX_EQUEUE || status == VBM_MUX_EPACKET)
        h.flags |= status << OGGMUX_FAIL_SHIFT;
    if (flush) {
        OggMuxPage pg;
        while (npages < d.max_pages && oggmux_pageout(h, lacing, gran, head, tail, body_head, 1, pg)) {
            pages[npages++] = pg;
            out_bytes += 27 + pg.nseg + pg.body_bytes;
        }
    }
    c.out_bytes = out_bytes;
    c.body_used = body_head;
    c.body_total = body_total;
    c.lace_used = head;
    c.lace_total = tail;
    c.npages = npages;
    c.nrows = taken;
    return status;
}

// the 27 header bytes of a page, CRC field zero
VBMX_HD void oggmux_page_header(const OggMuxPage &pg, int serialno, uint8_t *o)
{
    o[0] = 'O', o[1] = 'g', o[2] = 'g', o[3] = 'S';
    o[4] = 0;
    o[5] = (uint8_t)pg.flags;
    for (int i = 0; i < 8; i++) o[6 + i] = (uint8_t)(((unsigned long long)pg.granule >> (8 * i)) & 0xff);
    for (int i = 0; i < 4; i++) o[14 + i] = (uint8_t)(((uint32_t)serialno >> (8 * i)) & 0xff);
    for (int i = 0; i < 4; i++) o[18 + i] = (uint8_t)(((uint32_t)pg.pageno >> (8 * i)) & 0xff);
    for (int i = 0; i < 4; i++) o[22 + i] = 0;
    o[26] = (uint8_t)pg.nseg;
}

// ---- CRC: polynomial 0x04c11db7, not reflected, initial value 0, no final xor (doc/framing.html:363-366) -----------
// With these it is linear over GF(2): crc(A || B) = crc(A) * x^(8|B|) mod P  xor  crc(B).
VBMX_HD uint32_t oggmux_crc_entry(uint32_t i)
{
    uint32_t r = i << 24;
    for (int k = 0; k < 8; k++) r = (r & 0x80000000u) ? (r << 1) ^ 0x04c11db7u : (r << 1);
    return r;
}

// a * b mod P, bit 31 of a word = x^31
VBMX_HD uint32_t oggmux_gfmul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 31; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x80000000u) ? 0x04c11db7u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

#define OGGMUX_NPOW 17   // a page is at most 27 + 255 + 255 * 255 = 65307 bytes < 2^17
struct OggMuxPow {
    uint32_t x[OGGMUX_NPOW];   // x^(8 * 2^k) mod P
};

VBMX_HD OggMuxPow oggmux_pow_table()
{
    OggMuxPow p;
    p.x[0] = 0x100u;
    for (int k = 1; k < OGGMUX_NPOW; k++) p.x[k] = oggmux_gfmul(p.x[k - 1], p.x[k - 1]);
    return p;
}

// the CRC of a run as it stands when n more bytes follow it: crc * x^(8n) mod P
VBMX_HD uint32_t oggmux_crc_shift(const OggMuxPow &p, uint32_t crc, uint32_t n)
{
    for (int k = 0; k < OGGMUX_NPOW && n; k++, n >>= 1)
        if (n & 1u) crc = oggmux_gfmul(crc, p.x[k]);
    return crc;
}
