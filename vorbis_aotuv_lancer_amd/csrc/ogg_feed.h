// Incremental Ogg demux for many live streams: the rules of demux() in capi_stream.cpp applied as the bytes arrive, written
// once for the host twin (vbm_host_ogg_feed_*) and the device kernels (ogg_feed.hip) over a fixed-size state per stream
// slot.  The page walk (oggdmx_walk_step, whose "not all here yet" is what a feed carries), the carried counts, the CRC,
// the packet-end rule and the body split are those of ogg_demux.h.
//
// A stream's body bytes are numbered over its whole life, as ogg_demux.h numbers them over a file: body byte b of the
// stream, packet q of the stream.  A call sees the run "carried page tail + chunk", takes the whole pages from it and
// leaves the rest as the next tail.  With S = the end of the last packet completed before the call (the end of the
// third header packet while fewer than three were complete) and E = the end of the last packet completed by it, the
// call's payload for the stream is body bytes [S, E): those below the first new page are the carried part of the open
// packet (OggFeedState::body - last_end of them, kept in the slot's open store), the others lie on the call's pages.
// Body bytes below the end of the third packet go to the slot's header store at their own number, an open header packet
// included, so the header store needs no carry of its own.
//
// Per slot: OggFeedState (72 B) + max_page_carry + max_packet_bytes + header_cap bytes.  Per call, sized at create: the
// work buffer that holds every listed stream's run, max_call_bytes + max_streams * max_page_carry bytes (stream i of the
// list starts at chunk_offset[i] - chunk_offset[0] + i * max_page_carry), and the page records.  A run whose tail is
// an incomplete page holds at most chunk / 27 + 1 pages, so stream i's records start at slot
// (chunk_offset[i] - chunk_offset[0]) / 27 + i and there are max_call_bytes / 27 + max_streams + 1 of them.
//
// Resync mode (oggfeed_rs_walk; the rules: include/vorbis_mi355x.h, "Resync mode") keeps the same numbering and the same
// page records, so gather, fill and commit are those of the strict mode.  A link start numbers the new link's body bytes
// and packets from 0 again.  A discontinuity page rewinds the numbering to last_end, which empties the open store (an
// open packet's bytes lie at their distance from last_end), and a continued discontinuity page folds its front skip
// into its record: with `skip` leading body bytes that belong to no packet, body_before is `skip` below the rewound
// count, so the skipped bytes get numbers below S (no payload), the first kept byte gets number S, and the lacing value
// that ends the skipped part counts as the end of the packet in front of the call's first (pkt_before one less), which
// rewrites that packet's end offset, the call's first CSR entry, with the value it has.  Such a record is marked
// (OggDmxPage::pad), because its numbers below S are not header bytes.  Per slot 16 B more (OggFeedLink).
//
// Multiplexed mode (VBM_OGG_FEED_MULTIPLEXED, alone or with the resync mode): the rule of ogg_select.h applied page by
// page in front of either walk, with its predicates (oggsel_wants_mark, oggsel_choose, oggsel_is_mark) over the two words
// a slot carries (OggFeedMux, 8 B more per slot; the chosen serial number is the one the slot tracks, OggDmxCounts::
// serial).  For every WHOLE page the walk meets, in this order (oggfeed_mux_page):
//     head = (flags & 2), or the page is the first the slot meets (as pos == begin in ogg_select.h);
//     head && past_heads: a new group starts: past_heads = 0, chosen = 0;
//     !head:              past_heads = 1;
//     head && !chosen, the body has 7 bytes or more and begins 01 'v' 'o' 'r' 'b' 'i' 's' (read only now that the body
//                         is known to lie in the run): chosen = 1, and the page is the stream's own;
//     the page is KEPT if and only if chosen and its serial number is the chosen one (a head page that sets chosen is);
//     otherwise it is foreign.
// A foreign page is stepped over whole: no page record, no body byte to any store, no CRC check in strict mode; it is
// counted (a resync feed reports the count in ignored_pages).  A kept page goes to the walk as if no other had been there.
// The group state moves on only with a page the walk has passed: a page at which a call stops is judged again by the
// next call, from the same state.
//   strict  the feed does what the strict feed does on the bytes ogg_select.h keeps (oggfeed_mux_step), with two
//           deviations that a live feed cannot avoid.  A position that does not parse as a page header (capture
//           pattern, version) once 27 bytes are there is VBM_EOGG whether or not a stream is chosen: there is no end
//           of file at which an unchosen tail could be dropped.  And a head page that has to show the mark is judged
//           once it is whole, not once its header is: the VBM_EOGG of a chain comes in the call that completes the
//           second group's Vorbis head page.  A page behind the heads with the chosen serial number is kept whatever
//           its body holds, so the walk judges its header at once, as without the flag.
//   resync  rule 1 is unchanged, and only a page with a good CRC reaches the group state.  Rule 2: a page is a link
//           start when it carries the beginning-of-stream flag and is kept; a foreign page, head or not, is ignored
//           and counted, and closes no link, drops no packet and sets no mark.  Rules 3 to 6 are untouched.
// A foreign page that is not whole yet is carried like any page, within max_page_carry.  Page records stay
// chunk / 27 + 1 per slot: foreign pages take none.
#pragma once
#include <limits.h>

#include "ogg_select.h"

struct OggFeedCaps {
    int max_page_carry, max_packet_bytes, header_cap;
};

struct OggFeedState {            // one stream slot between calls; all zero = a fresh slot
    OggDmxCounts cnt;            // over the pages taken so far
    int partial;                 // a packet is open at the end of the last page taken
    int status;                  // sticky: 0, VBM_EOGG, VBM_OGG_FEED_EBIG
    int tail;                    // bytes of the incomplete trailing page in the slot's tail store
    int done;                    // the `end` flag has been seen
};

static_assert(sizeof(OggFeedState) == 72, "OggFeedState is the slot's memory");

struct OggFeedCall {             // one listed stream of a scan, for fill and commit
    OggFeedState next;           // the slot's state once the call is committed
    long long at, pos_end;       // the run's first byte in the work buffer, the first byte behind its last whole page
    long long S, E;              // the call's payload in the stream's body bytes; S == E when it has none
    long long packets, payload_bytes, packet_base, payload_base;
    long long pkt_shift;         // audio packets completed before the call
    int npages;                  // whole pages taken
    int open_in;                 // bytes of the slot's open store that start the call's payload (0: none are used)
    int slot, pad;
};

struct OggFeedLink {             // resync mode: a slot's link between calls; all zero = no link yet
    int links;                   // link starts seen: the current link is links - 1 (reported as 0 before the first)
    int bad;                     // the link lost a page while its headers were open
    int eos;                     // the link has delivered its end-of-stream page
    int gap;                     // the next packet completed carries a gap mark
};

struct OggFeedRsCall {           // one listed stream of a resync scan, beside its OggFeedCall
    OggFeedLink next;            // the slot's link once the call is committed
    vbm_ogg_feed_events ev;
};

struct OggFeedHead {             // a whole page candidate
    int flags, nseg, body;       // header type, segments, body bytes (the sum of the lacing values)
    uint32_t serial, seq;
    uint32_t lace;               // device: this lane's four bytes of the 256 behind the header (for `mark`)
};

struct OggFeedMux {              // multiplexed mode: a slot's group between calls; all zero = a fresh slot
    int past_heads;              // bit 0: a page without the head flag has been met in the group (the inverse of
                                 // ogg_select.h's in_heads); bit 1: the slot has met a page
    int chosen;                  // the group has shown its Vorbis head page
};

static_assert(sizeof(OggFeedMux) == 8, "OggFeedMux is the slot's memory");

// One whole page against the group state (the rule: the head of this file).  serial: the one the slot tracks;
// sno, body: the page's; mark(): its first 7 body bytes are the mark, asked only when the rule wants them.  Moves mx on
// -> the page is kept
template <class Mark>
VBMX_HD bool oggfeed_mux_page(OggFeedMux &mx, uint32_t serial, int flags, uint32_t sno, int body, const Mark &mark)
{
    OggSelWalk w;
    w.in_heads = !(mx.past_heads & 1), w.chosen = mx.chosen != 0, w.serial = serial;
    w.info = vbm_ogg_select_info{};
    const bool head = (flags & 2) || !(mx.past_heads & 2);
    const bool shown = oggsel_wants_mark(w, head, body) && mark();
    const bool kept = oggsel_choose(w, head, sno, shown);
    mx.past_heads = (w.in_heads ? 0 : 1) | 2;
    mx.chosen = w.chosen;
    return kept;
}

// A strict multiplexed feed's run at pos, in front of the walk's own step:
//    1  a foreign page of len bytes, all here: to be stepped over (nm: the group state behind it)
//    0  the walk's own step goes on from here: the run is used up, or the page is kept (nm: the state once it is taken)
//   -1  no page header (27 bytes are here)
//   -2  the header, the lacing table or the body is not all in front of run_end
// No byte is read before it is known to lie in front of run_end.
VBMX_HD int oggfeed_mux_step(const uint8_t *work, long long pos, long long run_end, uint32_t serial, const OggFeedMux &mx,
                             OggFeedMux &nm, int &len)
{
    nm = mx;
    const long long left = run_end - pos;
    if (left <= 0) return 0;
    if (left < 27) return -2;
    const uint8_t *h = work + pos;
    if (!oggchain_header_ok(oggdmx_rd32(h), h[4])) return -1;
    const int flags = h[5], nseg = h[26];
    const uint32_t sno = oggdmx_rd32(h + 14);
    const auto none = [] { return false; };
    const bool head = (flags & 2) || !(mx.past_heads & 2);
    if (!head && oggfeed_mux_page(nm, serial, flags, sno, 0, none)) return 0;   // kept whatever its body holds
    if (!oggchain_lacing_fits(left, nseg)) return -2;
    int body = 0;
    for (int i = 0; i < nseg; i++) body += h[27 + i];
    if (!oggchain_body_fits(left, nseg, body)) return -2;
    len = 27 + nseg + body;
    if (!head) return 1;
    const uint8_t *b = h + 27 + nseg;                              // 7 bytes are there when asked for; the eighth may not be
    const auto mark = [b] {
        return oggsel_is_mark(oggdmx_rd32(b), (uint32_t)b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16));
    };
    return oggfeed_mux_page(nm, serial, flags, sno, body, mark) ? 0 : 1;
}

VBMX_HD int oggfeed_tail_in(const OggFeedState &st, const OggFeedCaps &caps)
{
    if (st.status || st.done) return 0;
    return st.tail < 0 ? 0 : (st.tail > caps.max_page_carry ? caps.max_page_carry : st.tail);
}

// a call that takes nothing
VBMX_HD void oggfeed_call_begin(const OggFeedState &st, long long at, int slot, OggFeedCall &c)
{
    c.next = st;
    c.at = c.pos_end = at;
    c.S = c.E = 0;
    c.packets = c.payload_bytes = c.packet_base = c.payload_base = 0;
    c.pkt_shift = (st.cnt.packets > 3 ? st.cnt.packets : 3) - 3;
    c.npages = c.open_in = 0;
    c.slot = slot, c.pad = 0;
}

// One stream, one call.  The run is work[at, run_end): whole pages are taken from it in order, at most `limit` of them,
// and recorded in pages[0, room).  bad_at_limit: the page after the first `limit` failed its CRC (the second walk of a
// stream, after the page-parallel CRC pass).  No byte is read before it is known to lie in front of run_end, and every
// page taken moves on by at least 27 bytes.  Fills `c` but for its bases.  MUX: the multiplexed mode; mx is the slot's
// group state and becomes the one behind the last page passed (`limit` counts recorded pages: foreign pages take no
// record, and the second walk of a stream passes the same foreign pages between them as the first).
template <bool MUX>
VBMX_HD void oggfeed_walk(const uint8_t *work, long long at, long long run_end, const OggFeedState &st,
                          const OggFeedCaps &caps, int end_flag, int limit, bool bad_at_limit, OggDmxPage *pages,
                          long long room, int slot, OggFeedCall &c, OggFeedMux &mx)
{
    oggfeed_call_begin(st, at, slot, c);
    if (st.status || st.done) return;                              // bytes for a failed or ended stream are ignored
    OggDmxWalk w;
    w.pos = at, w.end = run_end;
    w.cnt = st.cnt, w.partial = st.partial;
    int status = 0, n = 0;
    while (n < limit) {
        OggFeedMux nm = {};
        if (MUX) {
            int len = 0;
            const int f = oggfeed_mux_step(work, w.pos, run_end, w.cnt.serial, mx, nm, len);
            if (f == 1) {                                          // foreign: stepped over whole
                mx = nm;
                w.pos += len;
                continue;
            }
            if (f < 0) {
                if (f == -1) status = VBM_EOGG;
                break;
            }
        }
        const OggDmxWalk before = w;
        OggDmxPage pg;
        const int r = oggdmx_walk_step(work, w, pg);
        if (r != 1) {                                              // the run is used up, or its rest is carried (-2)
            if (r == -1) status = VBM_EOGG;
            break;
        }
        // the stores the page's body would go to.  Judged page by page, so that the outcome does not depend on where
        // the calls cut the stream.
        const long long hdr = before.cnt.packets >= 3 ? 0 : (w.cnt.packets >= 3 ? w.cnt.h2 : w.cnt.body);
        const long long open = w.cnt.packets >= 3 ? w.cnt.body - w.cnt.last_end : 0;
        const bool big = hdr > caps.header_cap || open > caps.max_packet_bytes;
        if (n >= room || big) {                                    // no room: cannot happen (a page is 27 bytes or more)
            w = before;
            status = n >= room ? VBM_EOGG : VBM_OGG_FEED_EBIG;
            break;
        }
        pages[n++] = pg;
        if (MUX) mx = nm;
    }
    if (bad_at_limit && n == limit) status = VBM_EOGG;
    long long tail = status ? 0 : run_end - w.pos;
    int done = 0;
    if (!status && end_flag) {
        if (tail > 0 || w.cnt.packets < 3) status = VBM_EOGG;      // a truncated page, fewer than three header packets
        tail = 0;
        done = 1;
    } else if (!status && tail > caps.max_page_carry) {
        status = VBM_OGG_FEED_EBIG;
        tail = 0;
    }
    c.npages = n;
    c.pos_end = w.pos;
    if (w.cnt.packets >= 3) {
        c.S = st.cnt.packets >= 3 ? st.cnt.last_end : w.cnt.h2;
        c.E = w.cnt.last_end;
        c.packets = w.cnt.packets - 3 - c.pkt_shift;
        c.payload_bytes = c.E - c.S;
        if (st.cnt.packets >= 3 && c.packets > 0) c.open_in = (int)(st.cnt.body - st.cnt.last_end);
    }
    c.next.cnt = w.cnt, c.next.partial = w.partial;
    c.next.status = status;
    c.next.tail = (int)tail;
    c.next.done = done;
}

VBMX_HD void oggfeed_info(const OggFeedCall &c, vbm_ogg_feed_info &fi)
{
    const OggDmxCounts &s = c.next.cnt;
    const bool ready = s.packets >= 3;
    fi.status = c.next.status;
    fi.headers_ready = ready ? 1 : 0;
    fi.header_bytes[0] = ready ? (int)s.h0 : 0;
    fi.header_bytes[1] = ready ? (int)(s.h1 - s.h0) : 0;
    fi.header_bytes[2] = ready ? (int)(s.h2 - s.h1) : 0;
    fi.serialno = s.seq ? s.serial : 0u;
    fi.packets = c.packets;
    fi.payload_bytes = c.payload_bytes;
    fi.packet_base = c.packet_base;
    fi.payload_base = c.payload_base;
    fi.pending = c.next.tail;
    fi.consumed = c.pos_end - c.at;
}

// The three views of a page of the call, in the terms of ogg_demux.h's fill:
//   payload  packet ends and body bytes [S, E) -> the caller's CSR (headers: none)
//   keep     body bytes below the end of the third packet -> the slot's header store, at their own number; body bytes
//            from E on -> the slot's open store, at their distance from E (as the "payload" of a file that starts at E)
VBMX_HD void oggfeed_ctx_payload(const uint8_t *work, const OggDmxPage &pg, const OggFeedCall &c, OggDmxPageCtx &x)
{
    oggdmx_page_fields(work, pg, x);
    x.pkt_before = pg.pkt_before - c.pkt_shift;
    const bool audio = c.next.cnt.packets >= 3;
    const long long b = pg.body_before + x.body_len;               // while the headers are open, all of the body is theirs
    x.H = audio ? c.S : b;
    x.E = audio ? c.E : b;
    x.packet_base = c.packet_base, x.payload_base = c.payload_base, x.header_base = 0;
}

VBMX_HD void oggfeed_ctx_keep(const uint8_t *work, const OggDmxPage &pg, const OggFeedCall &c, const OggFeedCaps &caps,
                              OggDmxPageCtx &hdr, OggDmxPageCtx &open)
{
    oggfeed_ctx_payload(work, pg, c, hdr);
    const bool audio = c.next.cnt.packets >= 3;
    const long long b = pg.body_before + hdr.body_len;
    hdr.H = hdr.E = audio ? c.next.cnt.h2 : b;                     // [.., H) -> header store; no payload part
    if (pg.pad) hdr.H = hdr.E = pg.body_before;                    // a front skip: its numbers are no header bytes
    hdr.header_base = (long long)c.slot * caps.header_cap;
    open = hdr;
    open.H = audio ? c.next.cnt.last_end : b;                      // [H, ..) -> open store
    open.E = b;
    open.payload_base = (long long)c.slot * caps.max_packet_bytes;
}

// ---- resync mode ---------------------------------------------------------------------------------------------------
VBMX_HD bool oggfeed_rs_capture(uint32_t w) { return w == 0x5367674fu; }   // "OggS", the first byte lowest

// One stream, one call, by the six rules of the resync mode.  The run is work[at, run_end), its first tail_in bytes the
// carried tail.  What looks at many bytes comes from `ops`, serial on the host and by the lanes of a wavefront on the
// device (there every argument and result is uniform over the wavefront, and so is every exit of the loop):
//   find(work, pos, end)   the first p in [pos, end - 4] with the capture pattern at work[p, p + 4), or -1
//   head(h, left, hd)      the candidate at h with `left` bytes in front of the run's end: 1 whole (hd filled), 0 no
//                          header (version), -2 the header, the lacing table or the body is not all here
//   crc(h, len)            the page carries its own checksum
//   mark(h, hd)            (multiplexed mode) the first 7 body bytes of the whole page hd at h are the mark of ogg_select.h
// MUX: the multiplexed mode; mx is the slot's group state and becomes the one behind the last page passed.
// No byte is read before it is known to lie in front of run_end; every turn of the loop moves pos on by one byte at least
// or leaves it.  Fills `c` but for its bases, and `r`.
template <bool MUX, class Ops>
VBMX_HD void oggfeed_rs_walk(const Ops &ops, const uint8_t *work, long long at, long long run_end, int tail_in,
                             const OggFeedState &st, const OggFeedLink &lk0, const OggFeedCaps &caps, int end_flag,
                             OggDmxPage *pages, long long room, int slot, OggFeedCall &c, OggFeedRsCall &r, OggFeedMux &mx)
{
    oggfeed_call_begin(st, at, slot, c);
    r.next = lk0;
    r.ev.link = lk0.links > 0 ? lk0.links - 1 : 0;
    r.ev.link_started = r.ev.gaps = 0;
    r.ev.link_bad = lk0.bad;
    r.ev.skipped_bytes = r.ev.ignored_pages = r.ev.left = 0;
    if (st.status || st.done) return;                              // bytes for a failed or ended stream are ignored
    OggDmxCounts cnt = st.cnt, base = st.cnt;                      // base: the counts the call's payload starts from
    OggFeedLink lk = lk0;
    int partial = st.partial, n = 0, status = 0;
    bool took = false, stopped = false, started = false;
    long long pos = at, skipped = 0, ignored = 0;
    // The page records of a call are sized for its chunk (chunk / 27 + 1 per slot).  The carried tail may hold whole
    // pages too: behind a candidate that claimed more bytes than it had (a truncated page, a damaged lacing table)
    // everything is carried until the claim is filled, and when its CRC then fails the walk meets them all at once.  So
    // a call takes chunk / 27 + 1 pages at most, one at least, and the next ends the walk as any stop of rule 5 does.
    const long long fit = (run_end - at - tail_in) / 27 + 1, most = fit < room ? fit : room;
    while (run_end - pos >= 4) {
        // 1 finding a page
        const long long p = ops.find(work, pos, run_end);
        if (p < 0) {                                               // the last three bytes may begin a capture pattern
            skipped += run_end - 3 - pos;
            pos = run_end - 3;
            break;
        }
        skipped += p - pos;
        pos = p;
        const uint8_t *h = work + pos;
        OggFeedHead hd = {};
        const int whole = ops.head(h, run_end - pos, hd);
        if (whole == -2) break;                                    // carried
        const int len = 27 + hd.nseg + hd.body;                    // (of a whole candidate)
        if (whole == 0 || !ops.crc(h, len)) {
            skipped++;
            pos++;
            continue;
        }
        // 2 whose page
        OggFeedMux nm = {};
        if (MUX) {
            nm = mx;
            const auto mark = [&] { return ops.mark(h, hd); };
            if (!oggfeed_mux_page(nm, cnt.serial, hd.flags, hd.serial, hd.body, mark)) {   // foreign, head or not
                mx = nm;
                ignored++;
                pos += len;
                continue;
            }
        }
        const bool start = (hd.flags & 2) != 0, cont = (hd.flags & 1) != 0;
        if (!start && (lk.links == 0 || lk.bad || lk.eos || hd.serial != cnt.serial)) {
            if (MUX) mx = nm;
            ignored++;
            pos += len;
            continue;
        }
        const bool disc = start ? cont : (hd.seq != cnt.seq || cont != (partial != 0));
        if (((start || disc) && took) || n >= most) {              // 5 only as the first page the call takes; records
            stopped = true;
            break;
        }
        OggDmxCounts pre = cnt;
        OggFeedLink nl = lk;
        int np = partial, from = 0, skip = 0, skip_end = 0;
        if (start) {                                               // 4 link start
            pre = OggDmxCounts{};
            nl.links++;
            nl.bad = nl.eos = 0;
            nl.gap = nl.links > 1;
            np = 0;
        }
        if (disc) {                                                // 3 discontinuity
            if (pre.packets < 3) {                                 // headers open: the link is bad, the page is used up
                nl.bad = 1;
                if (MUX) mx = nm;
                cnt = pre, lk = nl, partial = 0;
                started = started || start;
                if (start) base = pre;
                took = true;
                pos += len;
                continue;
            }
            pre.body = pre.last_end;                               // the open packet is dropped
            np = 0;
            nl.gap = 1;
            if (cont)
                while (from < hd.nseg && !skip_end) {
                    const int lv = h[27 + from++];
                    skip += lv;
                    skip_end = lv < 255;
                }
        }
        OggDmxCounts nc = pre;
        oggdmx_lacing(h, from, hd.nseg, nc, np);
        // the stores the page's body would go to, judged page by page as in the strict mode
        const long long hdr = pre.packets >= 3 ? 0 : (nc.packets >= 3 ? nc.h2 : nc.body);
        const long long open = nc.packets >= 3 ? nc.body - nc.last_end : 0;
        if (hdr > caps.header_cap || open > caps.max_packet_bytes) {
            status = VBM_OGG_FEED_EBIG;
            break;
        }
        OggDmxPage pg;
        pg.at = pos;
        pg.body_before = pre.body - skip;
        pg.pkt_before = pre.packets - skip_end;
        pg.len = len;
        pg.pad = skip > 0 || skip_end;
        pages[n++] = pg;
        if (start || disc) base = pre;
        started = started || start;
        cnt = nc;
        cnt.serial = hd.serial;
        cnt.seq = hd.seq + 1;
        partial = np;
        lk = nl;
        if (hd.flags & 4) lk.eos = 1;
        if (MUX) mx = nm;
        took = true;
        pos += len;
    }
    // 5 stops: what the walk did not visit stays the tail (carried bytes) or is reported as left (bytes of the chunk)
    const long long chunk_at = at + tail_in;
    long long tail = run_end - pos, left = 0;
    if (stopped) {
        tail = pos < chunk_at ? chunk_at - pos : 0;
        left = run_end - (pos < chunk_at ? chunk_at : pos);
    }
    if (status) tail = left = 0;
    int done = 0;
    if (!status && end_flag && !stopped) {                         // 6 a partial page is dropped; not at a stop: left > 0,
                                                                   // or whole pages of the tail are still unvisited
        skipped += tail;
        tail = 0;
        done = 1;
    } else if (!status && tail > caps.max_page_carry) {
        status = VBM_OGG_FEED_EBIG;
        tail = 0;
    }
    c.npages = n;
    c.pos_end = pos;
    c.pkt_shift = (base.packets > 3 ? base.packets : 3) - 3;
    if (cnt.packets >= 3) {
        c.S = base.packets >= 3 ? base.last_end : cnt.h2;
        c.E = cnt.last_end;
        c.packets = cnt.packets - 3 - c.pkt_shift;
        c.payload_bytes = c.E - c.S;
        if (base.packets >= 3 && c.packets > 0) c.open_in = (int)(base.body - base.last_end);
    }
    if (c.packets > 0 && lk.gap) {                                 // the call's first packet carries the mark
        r.ev.gaps = 1;
        lk.gap = 0;
    }
    c.next.cnt = cnt, c.next.partial = partial;
    c.next.status = status;
    c.next.tail = (int)tail;
    c.next.done = done;
    r.next = lk;
    r.ev.link = lk.links > 0 ? lk.links - 1 : 0;
    r.ev.link_started = started;
    r.ev.link_bad = lk.bad;
    r.ev.skipped_bytes = skipped;
    r.ev.ignored_pages = ignored;
    r.ev.left = left;
}

// the host's four: byte after byte
struct OggFeedSerialOps {
    const uint32_t *T;
    const OggMuxPow *pw;

    long long find(const uint8_t *work, long long pos, long long end) const
    {
        for (long long p = pos; p + 4 <= end; p++)
            if (oggfeed_rs_capture(oggdmx_rd32(work + p))) return p;
        return -1;
    }

    int head(const uint8_t *h, long long left, OggFeedHead &hd) const
    {
        if (left >= 5 && h[4] != 0) return 0;
        if (left < 27) return -2;
        hd.flags = h[5], hd.nseg = h[26];
        hd.serial = oggdmx_rd32(h + 14), hd.seq = oggdmx_rd32(h + 18);
        if (left - 27 < hd.nseg) return -2;
        hd.body = 0;
        for (int i = 0; i < hd.nseg; i++) hd.body += h[27 + i];
        return left - 27 - hd.nseg < hd.body ? -2 : 1;
    }

    bool crc(const uint8_t *h, int len) const { return oggdmx_page_crc_ok(T, *pw, h, len); }

    bool mark(const uint8_t *h, const OggFeedHead &hd) const
    {
        const uint8_t *b = h + 27 + hd.nseg;                       // asked for only when the body has 7 bytes or more
        return oggsel_is_mark(oggdmx_rd32(b), (uint32_t)b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16));
    }
};

VBMX_HD void oggfeed_rs_info(const OggFeedCall &c, const OggFeedRsCall &r, vbm_ogg_feed_info &fi)
{
    oggfeed_info(c, fi);
    fi.serialno = r.next.links ? c.next.cnt.serial : 0u;           // a sequence number may be any value here
}
