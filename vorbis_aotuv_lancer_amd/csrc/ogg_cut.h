// Sample windows of indexed streams cut into new Ogg Vorbis files with the packets left as they are: the rule, written
// once for the host twin (vbm_host_ogg_cut_ranges) and the device kernels (ogg_cut.hip).
//
// The rule.  Stream i of the store, start s, length L, in the store's output samples:
//   got = clamp(total_i - s, 0, L); got == 0: the output is empty, status 0.
//   k = the first packet with out_end > s, m = the packet that holds sample s + got - 1, pre = the last packet in front
//   of k with status 0: vbm_range_find (range_plan.h), the search of vbm_synthesis_ranges.  The file holds the stream's
//   header packets and the packets pre .. m unchanged, failed ones among them too.
//   The first packet of a Vorbis stream only primes the overlap, so pre gives nothing.  The decoder then drops from the
//   start what the first granule position does not account for, and stops at the granule position of the e_o_s packet
//   (vorbis_synthesis_blockin, reference lib/block.c:1084-1157: the first-page trim :1090-1115 under
//   `v->granulepos == -1`, the end trim :1121-1151).  So
//     packet j gets granule position out_end[j] - s, packet m gets `got` and e_o_s;
//     the first audio page ends with packet k (a forced flush), which makes k, not pre, carry the first granule
//     position; after it oggmux_pageout's rule (ogg_mux.h) pages k + 1 .. m, and everything goes out at e_o_s.
//   k == m: the one granule position is first and last at once, and block.c:1090-1115 reads it as an end trim.  The
//   start cannot be cut as well: it moves back to out_start[k], and the call reports start and length of every range.
//   The header pages are the host writer's (vbm_ogg_stream_*), given by the caller as sets that ranges may share (the
//   pages of a source file serve every cut of it) under any serial number: the range's serial number is written into
//   them and each page's CRC corrected by the linearity of the code (oggcut_reserial_crc), so the pages are what the
//   writer makes under the range's serial number.  The audio pages' numbers run on from them.
// Refused (VBM_OGG_CUT_ESHAPE, empty output): the file would not decode to the window.
//   (a) pre .. k do not share a page under the host writer's flush: more than 255 segments, or, with four packets and
//       more than 4096 bytes in front of one of them, the page the writer would end there;
//   (b) a packet j, k < j <= m, has begin[j] != 0: the source trimmed a start after output had begun;
//   (c) k == m and begin[k] != 0;
//   (d) the offsets of pre .. m are no CSR inside the store's data (negative, decreasing, past the end).
// Not covered: a hand-made store with e_o_s in front of a stream's last packet (its index ends the output there, and a
// cut across that packet is not what the source decodes to).
//
// The walk takes one packet at a time and keeps O(1) state: the page being filled (segments, body bytes, packets
// that end on it, the last one's granule position, where it began).  A page goes out
//   - in front of a packet, when more than 4096 body bytes and at least four ended packets lie on it
//     (oggmux_pageout's test holds only where the segment in front ends a packet);
//   - inside or behind a packet, at 255 segments;
//   - behind k (the flush) and behind m (e_o_s).
// Between packets that is the page oggmux_pageout finds over the whole lacing sequence, and the whole sequence gives
// the pages the packet-by-packet writer gives: a page is due on a prefix as soon as the prefix shows it.
//
// Workspace, for calls of up to R = max_ranges ranges and B = max_out_bytes output bytes.  Page slots: per range one
// for its header pages together, one for the first audio page, one for the page that empties the queue; every other
// page carries 255 segments (at least 27 + 255 = 282 bytes of output) or more than 4096 body bytes, so
//     slots <= 3 * R + B / 282                                                       (oggcut_max_pages)
// at 48 B each: 0.17 B per output byte.  Per range 24 B of counts and offsets and a 56 B record; the records and the header page
// sets go up through one pinned stage of R * 56 + max_header_bytes bytes (two slots).
#pragma once
#include <stdint.h>

#include "ogg_mux.h"

struct OggCutRange {      // one range as the host search leaves it
    long long s;          // the window's start (moved back to out_start[k] when k == m)
    long long got;        // its length; 0: empty output
    long long hdr_at;     // the range's header pages in the uploaded buffer
    int hdr_bytes, hdr_pages;
    int pre, k, m;        // packets of the store's CSR
    int serialno;
    int pad[2];
};

struct OggCutPage {       // one audio page
    long long granule;
    long long body_src;   // first body byte in the store's data
    long long out_at;     // the page in its range's output
    int nseg, body_bytes, flags, pageno;
    int pkt0, skip0;      // the packet of the first segment, and how many of its segments lie on earlier pages
};

VBMX_HD long long oggcut_max_pages(long long max_ranges, long long max_out_bytes)
{
    return 3 * max_ranges + max_out_bytes / 282;
}

struct OggCutWalk {
    int vals, acc, done;          // the page being filled: segments, body bytes, packets that end on it
    long long gran;               // granule position of the last of those
    int pkt0, skip0, open;        // where it began; 1: the page before ended inside a packet
    long long body0;
    int npages, pageno;           // audio pages out so far; the next page's number
    long long bytes;              // output bytes so far, header pages included
};

VBMX_HD void oggcut_begin(OggCutWalk &w, const OggCutRange &rg, long long body0)
{
    w.vals = w.acc = w.done = 0;
    w.gran = -1;
    w.pkt0 = rg.pre, w.skip0 = 0, w.open = 0;
    w.body0 = body0;
    w.npages = 0, w.pageno = rg.hdr_pages;
    w.bytes = rg.hdr_bytes;
}

// the page being filled goes out; the next begins at segment `skip` of packet `pkt`, body byte `body`
VBMX_HD void oggcut_page(OggCutWalk &w, int eos, int pkt, int skip, long long body, OggCutPage *pages, bool write)
{
    if (write) {
        OggCutPage pg;
        pg.granule = w.done ? w.gran : -1;
        pg.body_src = w.body0;
        pg.out_at = w.bytes;
        pg.nseg = w.vals, pg.body_bytes = w.acc;
        pg.flags = (w.open ? 0x01 : 0) | (eos ? 0x04 : 0);
        pg.pageno = w.pageno;
        pg.pkt0 = w.pkt0, pg.skip0 = w.skip0;
        pages[w.npages] = pg;
    }
    w.bytes += 27 + w.vals + w.acc;
    w.npages++, w.pageno++;
    w.open = skip != 0;
    w.vals = w.acc = w.done = 0;
    w.gran = -1;
    w.pkt0 = pkt, w.skip0 = skip, w.body0 = body;
}

// Packet j of the range, `bytes` long at byte `at` of the data, with out_end[j] and begin[j] of the index.
// -> 0, or VBM_OGG_CUT_ESHAPE: the range is refused
VBMX_HD int oggcut_packet(OggCutWalk &w, const OggCutRange &rg, int j, long long at, int bytes, long long out_end, int begin,
                          OggCutPage *pages, bool write)
{
    if ((j > rg.k || (j == rg.k && rg.k == rg.m)) && begin != 0) return VBM_OGG_CUT_ESHAPE;   // (b), (c)
    const int segs = bytes / 255 + 1;
    if (j <= rg.k) {
        // (a); a packet in front of k must leave k a segment
        if (w.vals + segs + (j < rg.k) > 255 || (w.acc > 4096 && w.done >= 4)) return VBM_OGG_CUT_ESHAPE;
    } else if (w.vals > 0 && w.acc > 4096 && w.done >= 4) {
        oggcut_page(w, 0, j, 0, at, pages, write);
    }
    const long long gran = j == rg.m ? rg.got : out_end - rg.s;
    int used = 0;                                   // segments of this packet on earlier pages
    while (segs - used > 255 - w.vals) {            // the page fills inside the packet: whole segments of 255
        const int take = 255 - w.vals;
        w.vals = 255, w.acc += take * 255;
        used += take;
        oggcut_page(w, 0, j, used, at + (long long)used * 255, pages, write);
    }
    w.acc += bytes - used * 255;
    w.vals += segs - used;
    w.done++;
    w.gran = gran;
    if (w.vals == 255 || j == rg.k || j == rg.m) oggcut_page(w, j == rg.m, j + 1, 0, at + bytes, pages, write);
    return 0;
}

// The CRC of a page of L bytes whose serial number (bytes 14 .. 17) changes from s0 to s1, c0 being its CRC before:
// the two pages differ in those four bytes alone (the CRC field counts as zero in both), and the code is linear
VBMX_HD uint32_t oggcut_reserial_crc(const OggMuxPow &pw, uint32_t c0, uint32_t s0, uint32_t s1, uint32_t L)
{
    const uint32_t d = s0 ^ s1;
    uint32_t crc = 0;
    for (int i = 0; i < 4; i++) crc = (crc << 8) ^ oggmux_crc_entry(((crc >> 24) ^ (d >> (8 * i))) & 0xff);
    return c0 ^ oggmux_crc_shift(pw, crc, L - 18);
}

VBMX_HD uint32_t oggcut_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// lacing values [0, nseg) of a page that begins at segment skip0 of a packet of `bytes` bytes: the packet's part.
// -> how many of the page's values it is; *last = its final value (the others are 255)
VBMX_HD int oggcut_lacing(int bytes, int skip, int room, int *last)
{
    const int segs = bytes / 255 + 1 - skip;
    if (segs > room) {
        *last = 255;
        return room;
    }
    *last = bytes % 255;
    return segs;
}
