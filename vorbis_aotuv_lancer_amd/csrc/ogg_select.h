// Which pages of a multiplexed Ogg file belong to its Vorbis stream: the rule, written once for the host twin
// (vbm_host_ogg_select), the device walk (ogg_select.hip: one wavefront per file) and the Python model of the tests.  A
// multiplexed file carries the pages of several logical streams interleaved, told apart by their serial numbers (the
// reference's doc/oggstream.html, "grouping"); with the foreign pages dropped it is a plain Vorbis file, or a plain
// chained one, for the split of ogg_chain.h and the demux of ogg_demux.h.  The choice is that of the reference's
// vorbisfile.c (_fetch_headers): the first stream of a group whose first packet is a Vorbis identification header.
//
// A file is bytes [begin, end).  From pos = begin, page after page, with the parse test of ogg_chain.h:
//     stop if fewer than 27 bytes are left, if the capture pattern is not "OggS", if the version byte is not 0,
//     if the nseg = h[26] lacing bytes are not all in front of end, or if the body (their sum) is not.
// The state is in_heads (true at begin), chosen (false at begin) and serial.  For the page at pos with flags fl, serial
// number s and `body` bytes of body, in this order:
//     head = (fl & 2) || pos == begin;
//     head && !in_heads: a new group starts (a chain boundary): in_heads = true, chosen = false;
//     !head:             in_heads = false;
//     head && !chosen, body >= 7 and the first 7 body bytes are 01 'v' 'o' 'r' 'b' 'i' 's' (read only now that the body
//                        is known to fit): chosen = true, serial = s;
//     the page is KEPT if and only if chosen && s == serial; otherwise it is foreign and dropped;
//     then pos += 27 + nseg + body.
// At a stop the tail [pos, end) is kept verbatim if chosen is true there, and dropped otherwise.
//
// The pass never fails and never judges.  CRC, page sequence, continuation flags, packet contents beyond those 7 bytes
// and the number of header packets are not looked at: they stay with the demux.  There is NO resync.  No byte outside
// [begin, end) is read, and every byte is known to lie in front of end before it is read.  Every step moves on by 27
// bytes or more, or stops, so the walk ends on any input.  What follows from the rule:
//   - the first Vorbis stream of a group wins; a second Vorbis stream in the same group is foreign;
//   - a foreign stream that reuses the serial number of an earlier group's chosen stream is still dropped (the new
//     group's first head page clears chosen, so nothing is kept until the group's own Vorbis head page, which sets the
//     serial number anew);
//   - a group with no Vorbis stream keeps nothing (Opus, video alone);
//   - a file in which every parsed page is kept (a plain Vorbis file or a plain chain of Vorbis links: each group's
//     first page body carries the mark) comes out byte for byte as it went in, tail included, at the same offsets.
//
// The output of a file is its kept RUNS back to back.  A run is a maximal sequence of adjacent kept pages; a kept tail
// that is not empty joins the run in front of it when its last page was kept, and is a run of its own otherwise.
// Workspace: a file that parsed P pages has n >= 27 P bytes.  With P = 0 nothing is chosen and there is no run.
// Otherwise two runs have a dropped page between them and every run but a lone tail holds a page; a lone tail needs a
// kept page (chosen is true) and a dropped page in front of it.  So there are at most P runs: P = 1 gives one, and
// P >= 2 gives at most P / 2 + 1 <= P.  P <= n / 27, and by the argument of ogg_demux.h file f may keep its records
// from slot (off[f] - off[0]) / 27 on without meeting its neighbour: max_bytes / 27 + 1 records of 24 B.
#pragma once
#include <stdint.h>

#include "ogg_chain.h"

struct OggSelRun {           // one run of a file
    long long src;           // its first byte in the call's data
    long long len;           // bytes, 1 at least
    long long dst;           // bytes of the file's output in front of it
};

struct OggSelWalk {          // one file while its pages are walked
    bool in_heads, chosen;
    uint32_t serial;
    bool open;               // a run is open: the last page was kept
    OggSelRun run;           // ... this one
    long long nruns;         // runs recorded
    vbm_ogg_select_info info;
};

// the first 8 body bytes as two little-endian words: they begin with the packet type 1 and "vorbis"
VBMX_HD bool oggsel_is_mark(uint32_t lo, uint32_t hi) { return lo == 0x726f7601u && (hi & 0xffffffu) == 0x736962u; }

VBMX_HD bool oggsel_is_head(int flags, long long pos, long long begin) { return (flags & 2) || pos == begin; }

VBMX_HD void oggsel_begin(OggSelWalk &w)
{
    w.in_heads = true, w.chosen = false, w.open = false;
    w.serial = 0;
    w.nruns = 0;
    w.run = OggSelRun{0, 0, 0};
    w.info = vbm_ogg_select_info{};
}

// The group state in front of the choice: does this page have to show the mark?  (Only then are body bytes read.)
VBMX_HD bool oggsel_wants_mark(OggSelWalk &w, bool head, int body)
{
    if (head && !w.in_heads) w.in_heads = true, w.chosen = false;
    if (!head) w.in_heads = false;
    return head && !w.chosen && body >= 7;
}

// ... and the choice: the page's serial number, and whether it showed the mark (false when it was not asked for)
// -> the page is kept
VBMX_HD bool oggsel_choose(OggSelWalk &w, bool head, uint32_t sno, bool mark)
{
    if (mark) {
        w.chosen = true, w.serial = sno;
        if (w.info.streams == 0) w.info.first_serial = sno;
        w.info.streams++;
    }
    const bool kept = w.chosen && sno == w.serial;
    if (head && !kept) w.info.foreign_streams++;
    return kept;
}

// The open run, if there is one, ends here: its record goes to runs[nruns] (written by `writer` alone: the device walk
// holds this state in every lane).  False when there is no room for it, which cannot happen (see above); as a second
// line of defence the file then keeps what its recorded runs hold, and the walk ends.
VBMX_HD bool oggsel_flush(OggSelWalk &w, OggSelRun *runs, long long room, bool writer)
{
    if (!w.open) return true;
    w.open = false;
    if (w.nruns >= room) {
        w.info.kept_bytes = w.run.dst;
        return false;
    }
    if (writer) runs[w.nruns] = w.run;
    w.nruns++;
    return true;
}

// len kept bytes at pos: they open a run or lengthen the open one
VBMX_HD void oggsel_keep(OggSelWalk &w, long long pos, long long len)
{
    if (!w.open) {
        w.open = true;
        w.run.src = pos, w.run.len = 0, w.run.dst = w.info.kept_bytes;
    }
    w.run.len += len;
    w.info.kept_bytes += len;
}

// the stop at pos: the tail is kept if a stream is chosen there
VBMX_HD void oggsel_stop(OggSelWalk &w, long long pos, long long end)
{
    if (w.chosen && end > pos) oggsel_keep(w, pos, end - pos);
}

// file [begin, end) one byte after the other: its runs -> runs[0 ...] (room for `room` of them), its counts -> info;
// returns the number of runs
VBMX_HD long long oggsel_walk_file(const uint8_t *data, long long begin, long long end, OggSelRun *runs, long long room,
                                   vbm_ogg_select_info &info)
{
    OggSelWalk w;
    oggsel_begin(w);
    long long pos = begin;
    bool link, room_left = true;
    while (room_left) {
        const int len = oggchain_step(data, begin, pos, end, link);
        if (!len) break;
        const uint8_t *h = data + pos;
        const int nseg = h[26], body = len - 27 - nseg;
        const bool head = oggsel_is_head(h[5], pos, begin);
        bool mark = false;
        if (oggsel_wants_mark(w, head, body)) {
            const uint8_t *b = h + 27 + nseg;                      // 7 bytes are there; the eighth may not be: not read
            mark = oggsel_is_mark(oggdmx_rd32(b), (uint32_t)b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16));
        }
        if (oggsel_choose(w, head, oggdmx_rd32(h + 14), mark)) {
            oggsel_keep(w, pos, len);
            w.info.kept_pages++;
        } else {
            w.info.foreign_pages++;
            room_left = oggsel_flush(w, runs, room, true);
        }
        pos += len;
    }
    if (room_left) {
        oggsel_stop(w, pos, end);
        oggsel_flush(w, runs, room, true);
    }
    info = w.info;
    return w.nruns;
}

// the run of a file's `nruns` that holds byte `at` of its output: the last r with runs[r].dst <= at
VBMX_HD long long oggsel_run_of(const OggSelRun *runs, long long nruns, long long at)
{
    long long lo = 0, hi = nruns - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (runs[mid].dst <= at) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
