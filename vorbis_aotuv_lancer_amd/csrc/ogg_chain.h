// Where the links of a chained Ogg file start: the rule, written once for the host twin (vbm_host_ogg_chain_split), the
// device walk (ogg_chain.hip: one wavefront per file) and any later caller that sees a file's bytes in order.  A chained
// file is whole logical streams back to back (the reference's doc/oggstream.html, "chaining"); cut at the link starts
// it is a batch of files for the demux of ogg_demux.h, which judges each link on its own bytes alone.
//
// A file is bytes [begin, end).  Link 0 starts at begin: in every file, an empty one included, and whatever its first
// page's flags say.  From pos = begin, page after page:
//     stop if fewer than 27 bytes are left, if the capture pattern is not "OggS", if the version byte is not 0,
//     if the nseg = h[26] lacing bytes are not all in front of end, or if the body (their sum) is not;
//     otherwise, if h[5] & 2 (beginning of stream) and pos != begin, a link starts at pos;
//     then pos += 27 + nseg + body.
// Link k is [start_k, start_k+1), the last one runs to end.
//
// The split never fails and never judges.  CRC, serial number, page sequence and the continuation flag are not looked
// at: they stay with the demux of each link.  After a stop the rest of the file belongs to the last link found, and the
// demux rejects that link as it would reject those bytes as a file.  There is NO resync: nothing is searched for behind
// a page that does not parse.  No byte outside [begin, end) is read, and every byte is known to lie in front of end
// before it is read.  Every step moves on by 27 bytes or more, or stops, so the walk ends on any input.
//
// Workspace: link 0 needs no record (it starts at begin).  Every later link starts at a page that has a page of the same
// file in front of it, so a file of n bytes has at most n / 27 - 1 of them, and by the argument of ogg_demux.h file f
// may keep them from slot (off[f] - off[0]) / 27 on without meeting its neighbour: max_bytes / 27 + 1 slots of 8 B.
#pragma once
#include <stdint.h>

#include "ogg_demux.h"

// the fixed part of a header, 27 bytes that are known to be there: false = stop
VBMX_HD bool oggchain_header_ok(uint32_t capture, int version)
{
    return capture == 0x5367674fu && version == 0;                 // "OggS" as a little-endian word
}

// `left` bytes from the page's first to the file's end: the lacing table is all there
VBMX_HD bool oggchain_lacing_fits(long long left, int nseg) { return left - 27 >= nseg; }

// ... and so is the body
VBMX_HD bool oggchain_body_fits(long long left, int nseg, int body) { return left - 27 - nseg >= body; }

VBMX_HD bool oggchain_starts_link(int flags, long long pos, long long begin) { return (flags & 2) && pos != begin; }

// The page at pos of the file [begin, end), one byte after the other: its length (27 or more) and whether a link
// starts with it, or 0 for a stop.
VBMX_HD int oggchain_step(const uint8_t *data, long long begin, long long pos, long long end, bool &starts)
{
    const long long left = end - pos;
    if (left < 27) return 0;
    const uint8_t *h = data + pos;
    if (!oggchain_header_ok(oggdmx_rd32(h), h[4])) return 0;
    const int nseg = h[26];
    if (!oggchain_lacing_fits(left, nseg)) return 0;
    int body = 0;
    for (int i = 0; i < nseg; i++) body += h[27 + i];
    if (!oggchain_body_fits(left, nseg, body)) return 0;
    starts = oggchain_starts_link(h[5], pos, begin);
    return 27 + nseg + body;
}

// file f of a call: the starts of its links 1, 2, ... -> starts[0 ...] (room for `room` of them); returns the number of
// its links, 1 at least
VBMX_HD long long oggchain_walk_file(const uint8_t *data, long long begin, long long end, long long *starts, long long room)
{
    long long pos = begin, extra = 0;
    bool link;
    while (int len = oggchain_step(data, begin, pos, end, link)) {
        if (link) {
            if (extra >= room) break;                              // cannot happen (see above): second line of defence
            starts[extra++] = pos;
        }
        pos += len;
    }
    return 1 + extra;
}

// link j of the batch: link k = j - file_links[f] of file f
VBMX_HD long long oggchain_link_start(const long long *off, const long long *file_links, const long long *starts,
                                      int nfiles, long long j)
{
    long long k;
    const int f = oggdmx_entry_of_page(file_links, nfiles, j, k);
    return k == 0 ? off[f] : starts[oggdmx_first_slot(off, f) + k - 1];
}
