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
#pragma once
#include <limits.h>

#include "ogg_demux.h"

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

VBMX_HD int oggfeed_tail_in(const OggFeedState &st, const OggFeedCaps &caps)
{
    if (st.status || st.done) return 0;
    return st.tail < 0 ? 0 : (st.tail > caps.max_page_carry ? caps.max_page_carry : st.tail);
}

// One stream, one call.  The run is work[at, run_end): whole pages are taken from it in order, at most `limit` of them,
// and recorded in pages[0, room).  bad_at_limit: the page after the first `limit` failed its CRC (the second walk of a
// stream, after the page-parallel CRC pass).  No byte is read before it is known to lie in front of run_end, and every
// page taken moves on by at least 27 bytes.  Fills `c` but for its bases.
VBMX_HD void oggfeed_walk(const uint8_t *work, long long at, long long run_end, const OggFeedState &st,
                          const OggFeedCaps &caps, int end_flag, int limit, bool bad_at_limit, OggDmxPage *pages,
                          long long room, int slot, OggFeedCall &c)
{
    c.next = st;
    c.at = c.pos_end = at;
    c.S = c.E = 0;
    c.packets = c.payload_bytes = c.packet_base = c.payload_base = 0;
    c.pkt_shift = (st.cnt.packets > 3 ? st.cnt.packets : 3) - 3;
    c.npages = c.open_in = 0;
    c.slot = slot, c.pad = 0;
    if (st.status || st.done) return;                              // bytes for a failed or ended stream are ignored
    OggDmxWalk w;
    w.pos = at, w.end = run_end;
    w.cnt = st.cnt, w.partial = st.partial;
    int status = 0, n = 0;
    while (n < limit) {
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
    hdr.header_base = (long long)c.slot * caps.header_cap;
    open = hdr;
    open.H = audio ? c.next.cnt.last_end : b;                      // [H, ..) -> open store
    open.E = b;
    open.payload_base = (long long)c.slot * caps.max_packet_bytes;
}
