// Tolerant demux of many whole Ogg files at once: rules 1 to 4 and 6 of the resync feed (include/vorbis_mi355x.h, "Resync
// mode"; ogg_feed.h, oggfeed_rs_walk) applied to a file pushed whole with `end`, written once for the host twin
// (vbm_host_ogg_resync_*) and the device kernels (ogg_resync.hip).  Rule 5 (stops, one link per call) and the slot
// capacities do not exist here.  Rules 2 to 4 are stated a second time below (oggrs_resolve_file) and ogg_feed.h is left
// as it is: the feed's walk carries its stops, its capacities and the multiplexed mode through the same loop, and the code
// generated for k_feed_resync_walk was not to move.
//
// What makes rule 1 parallel: whether a position holds the capture pattern, and what the candidate page there claims and
// whether its checksum holds, depend on the file's bytes alone, not on the walk.  So every "OggS" of the batch becomes a
// candidate (found by all lanes over the joined buffer), every candidate is judged on its own (one wavefront each:
// version, claimed size against the file's end, CRC, and a summary of its lacing table), and the walk that is left, the
// resolve, visits a file's candidate RECORDS in position order and never a file byte: it skips the candidates below the
// walk position (they lie inside a good page that was taken or ignored), stops at one whose claim runs past the file's
// end, moves on by one byte at a bad one and by the page's size at a good one, and applies rules 2 to 4 to the good ones.
//
// The numbering of body bytes and packets is ogg_demux.h's, per link: a link that completed its three header packets is
// an entry, H = the end of its third packet, E = the end of its last completed packet.  A discontinuity rewinds the
// numbering to the end of the last completed packet.  The feed can leave the dropped packet's bytes in place because a
// discontinuity page is the first of a call; here the pages in front of it are part of the same fill, so the resolve
// clips them (OggRsSide::keep) and no two pages of an entry write the same payload byte.  A continued discontinuity page
// is recorded as the feed records it (OggDmxPage::pad, body_before and pkt_before below the rewound counts), and its
// leading segments, which belong to no packet, are counted in OggRsSide (from, skip, skip_end) so that the fill starts
// behind them.
//
// Workspace, sized at create from max_files / max_bytes / max_candidates: a page taken, and an entry, each use up a
// candidate of their file, so file f's page records, side records and entries start at the number of its first candidate
// and none of them needs a scan before the resolve.  Per candidate 56 + 32 + 32 + 64 + 64 = 248 bytes; per 16 KB of input
// two counts of the search.
#pragma once
#include "ogg_demux.h"

constexpr int kRsTileDwords = 4096;      // a search tile: 16 KB of aligned dwords, four rows of 256 lanes x 4 dwords
constexpr int kRsRowDwords = 1024;

enum { OGGRS_NO = 0, OGGRS_GOOD = 1, OGGRS_END = 2 };

struct OggRsCand {               // one capture pattern whose four bytes lie in one file
    long long at;                // its first byte in the call's data
    int file;
    int len;                     // GOOD: 27 + nseg + body
    uint32_t serial, seq;
    int body;                    // the sum of the lacing values
    int nends;                   // lacing values below 255: packets that end on the page
    int last_end;                // body bytes through the last of them
    int e0, e1, e2;              // ... through the first three
    uint8_t verdict;             // NO: version or CRC (the walk moves on one byte); END: the claim runs past the file's end
    uint8_t flags, nseg;
    uint8_t partial;             // the last lacing value is 255
    int pad;
};

static_assert(sizeof(OggRsCand) == 56, "OggRsCand is workspace memory");

struct OggRsSide {               // beside a page record
    int entry;                   // the file's entry the page belongs to
    int from, skip, skip_end;    // a continued discontinuity page: leading segments / body bytes that belong to no packet,
                                 // and whether a lacing value below 255 ended them
    int nends;                   // packets that end on the page behind them
    int keep;                    // body bytes behind `skip` that are some packet's: the rest was dropped by a discontinuity
    long long gap_pkt;           // the entry's audio packet, completed on this page, that carries a gap mark; -1: none
};

static_assert(sizeof(OggRsSide) == 32, "OggRsSide is workspace memory");

VBMX_HD bool oggrs_capture(uint32_t w) { return w == 0x5367674fu; }   // "OggS", the first byte lowest

// The candidate at c.at, whose file ends at file_end, byte after byte (the host's judge; the device's: rs_wave_judge).
// No byte is read before it is known to lie in front of file_end.
VBMX_HD void oggrs_judge(const uint32_t *T, const OggMuxPow &pw, const uint8_t *data, long long file_end, OggRsCand &c)
{
    const uint8_t *h = data + c.at;
    const long long left = file_end - c.at;
    c.len = c.body = c.nends = c.last_end = c.e0 = c.e1 = c.e2 = 0;
    c.serial = c.seq = 0;
    c.flags = c.nseg = c.partial = 0;
    c.pad = 0;
    c.verdict = OGGRS_NO;
    if (left >= 5 && h[4] != 0) return;                            // stream structure version
    c.verdict = OGGRS_END;
    if (left < 27) return;
    const int nseg = h[26];
    if (left - 27 < nseg) return;
    int body = 0, ends = 0;
    for (int i = 0; i < nseg; i++) {
        const int lv = h[27 + i];
        body += lv;
        if (lv < 255) {
            if (ends == 0) c.e0 = body;
            if (ends == 1) c.e1 = body;
            if (ends == 2) c.e2 = body;
            ends++;
            c.last_end = body;
        }
        c.partial = lv == 255;
    }
    if (left - 27 - nseg < body) return;
    c.nseg = (uint8_t)nseg;
    c.body = body;
    c.nends = ends;
    c.len = 27 + nseg + body;
    c.flags = h[5];
    c.serial = oggdmx_rd32(h + 14), c.seq = oggdmx_rd32(h + 18);
    c.verdict = oggdmx_page_crc_ok(T, pw, h, c.len) ? OGGRS_GOOD : OGGRS_NO;
}

struct OggRsLink {               // the link the resolve is in
    int links, bad, eos, gap;    // as OggFeedLink
    long long first;             // the first of its page records
};

// The link ends: with its three header packets complete it is the file's next entry, otherwise its page records go.
VBMX_HD void oggrs_close_link(const OggDmxCounts &c, OggRsLink &lk, long long &n, long long &ne, vbm_ogg_file_info *ent)
{
    if (lk.links > 0 && !lk.bad && c.packets >= 3) {
        vbm_ogg_file_info fi;
        fi.status = 0;
        fi.pages = (int)(n - lk.first);
        fi.serialno = c.serial;
        fi.header_bytes[0] = (int)c.h0;
        fi.header_bytes[1] = (int)(c.h1 - c.h0);
        fi.header_bytes[2] = (int)(c.h2 - c.h1);
        fi.packets = c.packets - 3;
        fi.payload_bytes = c.last_end - c.h2;
        fi.packet_base = fi.payload_base = fi.header_base = 0;
        ent[ne++] = fi;
    } else {
        n = lk.first;
    }
    lk.first = n;
}

// One file, bytes [begin, end) of the call's data, from its candidates cand[0, ncand) in position order, judged.  Rule 1's
// bookkeeping and rules 2 to 4; touches no file byte.  pages, side, ent: the file's records, room for ncand each (a page
// taken and an entry each use up a candidate).  -> npages, nent, ev.
VBMX_HD void oggrs_resolve_file(const OggRsCand *cand, long long ncand, long long begin, long long end, OggDmxPage *pages,
                                OggRsSide *side, vbm_ogg_file_info *ent, long long &npages, long long &nent,
                                vbm_ogg_resync_events &ev)
{
    OggDmxCounts cnt = OggDmxCounts{};
    OggRsLink lk = {0, 0, 0, 0, 0};
    int partial = 0;
    long long pos = begin, n = 0, ne = 0, good_bytes = 0;
    ev.links_started = ev.links_bad = 0;
    ev.gaps = ev.skipped_bytes = ev.ignored_pages = ev.pages = 0;
    for (long long i = 0; i < ncand; i++) {
        const OggRsCand &c = cand[i];
        // 1 finding a page
        if (c.at < pos) continue;                                  // inside a good page: never looked at
        pos = c.at;
        if (c.verdict == OGGRS_END) break;                         // 6 a partial page, and all behind it, is dropped
        if (c.verdict == OGGRS_NO) {
            pos++;
            continue;
        }
        good_bytes += c.len;
        pos += c.len;
        // 2 whose page
        const bool start = (c.flags & 2) != 0, cont = (c.flags & 1) != 0;
        if (!start && (lk.links == 0 || lk.bad || lk.eos || c.serial != cnt.serial)) {
            ev.ignored_pages++;
            continue;
        }
        ev.pages++;
        const bool disc = start ? cont : (c.seq != cnt.seq || cont != (partial != 0));
        OggDmxCounts pre = cnt;
        int np = partial;
        if (start) {                                               // 4 link start
            oggrs_close_link(cnt, lk, n, ne, ent);
            pre = OggDmxCounts{};
            lk.links++;
            lk.bad = lk.eos = 0;
            lk.gap = lk.links > 1;
            np = 0;
            ev.links_started++;
        }
        int from = 0, skip = 0, skip_end = 0;
        if (disc) {                                                // 3 discontinuity
            if (pre.packets < 3) {                                 // headers open: the link is bad, the page is used up
                lk.bad = 1;
                cnt = pre, partial = 0;
                n = lk.first;
                continue;
            }
            // the open packet is dropped: its bytes on the pages in front lose their place
            for (long long j = n - 1; j >= lk.first; j--) {
                const long long b0 = pages[j].body_before + side[j].skip;
                if (b0 + side[j].keep <= pre.last_end) break;
                side[j].keep = (int)(pre.last_end > b0 ? pre.last_end - b0 : 0);
            }
            pre.body = pre.last_end;
            np = 0;
            lk.gap = 1;
            if (cont) {                                            // the leading segments belong to no packet
                skip_end = c.nends > 0;
                skip = skip_end ? c.e0 : c.body;
                from = skip_end ? c.e0 / 255 + 1 : c.nseg;
            }
        }
        OggDmxCounts nc = pre;                                     // oggdmx_lacing from segment `from`, by the summary
        const int ends = c.nends - skip_end;
        nc.body += c.body - skip;
        nc.packets += ends;
        if (ends > 0) nc.last_end = pre.body + (c.last_end - skip);
        if (pre.packets < 3) {                                     // (no skip here: a discontinuity made the link bad)
            const int e[3] = {c.e0, c.e1, c.e2};
            for (int j = 0; j < 3 && j < ends; j++) {
                const long long q = pre.packets + j;
                if (q == 0) nc.h0 = pre.body + e[j];
                if (q == 1) nc.h1 = pre.body + e[j];
                if (q == 2) nc.h2 = pre.body + e[j];
            }
        }
        if (c.nseg > from) np = c.partial;
        if (n >= ncand) break;                                     // cannot happen: a page taken uses up a candidate
        OggDmxPage pg;
        pg.at = c.at;
        pg.body_before = pre.body - skip;
        pg.pkt_before = pre.packets - skip_end;
        pg.len = c.len;
        pg.pad = skip > 0 || skip_end;
        OggRsSide sd;
        sd.entry = (int)ne;
        sd.from = from, sd.skip = skip, sd.skip_end = skip_end;
        sd.nends = ends;
        sd.keep = c.body - skip;
        sd.gap_pkt = -1;
        const long long first_audio = pre.packets > 3 ? pre.packets : 3;
        if (lk.gap && nc.packets > first_audio) {                  // the first audio packet completed carries the mark
            sd.gap_pkt = first_audio - 3;
            lk.gap = 0;
            ev.gaps++;
        }
        pages[n] = pg;
        side[n] = sd;
        n++;
        cnt = nc;
        cnt.serial = c.serial;
        cnt.seq = c.seq + 1;
        partial = np;
        if (c.flags & 4) lk.eos = 1;
    }
    oggrs_close_link(cnt, lk, n, ne, ent);
    npages = n;
    nent = ne;
    ev.links_bad = ev.links_started - (int)ne;
    ev.skipped_bytes = (end - begin) - good_bytes;
}

// A page of an entry as the fill of ogg_demux.h sees it, behind the segments and bytes that belong to no packet.  The
// body's source starts c.h + 27 + c.nseg + sd.skip: oggrs_body_split.
VBMX_HD void oggrs_page_ctx(const uint8_t *data, const OggDmxPage &pg, const OggRsSide &sd, const vbm_ogg_file_info &fi,
                            OggDmxPageCtx &c)
{
    oggdmx_page_ctx(data, pg, fi, c);                              // flags and granule position: the page's own header
    c.h += sd.from;
    c.nseg -= sd.from;
    c.body_len = sd.keep;
    c.body_before += sd.skip;
    c.pkt_before += sd.skip_end;
}

VBMX_HD OggDmxSplit oggrs_body_split(const OggDmxPageCtx &c, const OggRsSide &sd, const OggDmxOut &o)
{
    OggDmxSplit s = oggdmx_body_split(c, o);
    s.src_h += sd.skip;
    s.src_p += sd.skip;
    return s;
}

// the gap marks of the audio packets that end on the page: entry packets [first, last)
VBMX_HD void oggrs_gap_range(const OggDmxPageCtx &c, const OggRsSide &sd, long long &first, long long &last)
{
    first = (c.pkt_before > 3 ? c.pkt_before : 3) - 3;
    last = c.pkt_before + sd.nends - 3;
}

// the first candidate at or behind byte `at`: cand[0, n) is in position order
VBMX_HD long long oggrs_lower_bound(const OggRsCand *cand, long long n, long long at)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cand[mid].at < at) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
