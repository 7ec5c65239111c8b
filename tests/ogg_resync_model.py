"""The six rules of the resync feed (include/vorbis_mi355x.h, "Resync mode") restated byte-serially in Python: a slot
keeps bytes, Python lists and bytearrays, not the product's counts and page records, and the CRC is a plain table loop
(ogg_pages.page_crc).  Nothing here is shared with the product.  Slot.call() is one push of one slot; run() drives a
whole byte string through a list of cut points and pushes what a call left again, as OggFeed.push_all does."""
import struct

from tests.ogg_pages import page_crc


class Link:
    def __init__(self):
        self.headers, self.packets, self.granulepos, self.eos, self.gap = [], [], [], [], []


class Slot:
    def __init__(self):
        self.tail = b""
        self.links = []               # every link started so far
        self.serial = self.seq = 0
        self.open = None              # the bytes of the open packet; None: no packet is open
        self.npk = 0                  # packets the current link has completed
        self.bad = self.eos = self.gap = self.done = False

    # What a mode with a rule of its own between rule 1 (a whole page with a good CRC) and rule 2 (whose page) overrides;
    # ogg_feed_mux_cases.MuxSlot does.  A page the call stops at reaches none of the last three: the next call judges
    # it again.
    def foreign(self, page, nseg, bos, serial):
        """-> the page is not for rule 2 to judge: it is ignored"""
        return False

    def passed(self):
        """the page went by, ignored by rule 2 or taken"""

    def link_started(self):
        """the page taken starts a link"""

    def page_taken(self, serial):
        """the page taken goes on to its packets"""

    def call(self, chunk, end=False):
        """-> {packets: [(bytes, granulepos, eos, gap)], link, link_started, link_bad, gaps, skipped, ignored, left,
        headers_ready}"""
        out, skipped, ignored, left = [], 0, 0, 0
        started = stopped = took = False
        taken = 0
        if not self.done:
            run, carried, pos = self.tail + bytes(chunk), len(self.tail), 0
            while len(run) - pos >= 4:
                p = run.find(b"OggS", pos)
                if p < 0:
                    skipped += len(run) - 3 - pos
                    pos = len(run) - 3
                    break
                skipped += p - pos
                pos = p
                have = len(run) - pos
                if have >= 5 and run[pos + 4] != 0:
                    skipped, pos = skipped + 1, pos + 1
                    continue
                if have < 27 or have < 27 + run[pos + 26]:
                    break
                nseg = run[pos + 26]
                lacing = list(run[pos + 27:pos + 27 + nseg])
                size = 27 + nseg + sum(lacing)
                if have < size:
                    break
                page = run[pos:pos + size]
                flags, granule, serial, seq, crc = struct.unpack_from("<BqIII", page, 5)
                if page_crc(page) != crc:
                    skipped, pos = skipped + 1, pos + 1
                    continue
                bos, cont = bool(flags & 2), bool(flags & 1)
                if self.foreign(page, nseg, bos, serial):
                    ignored, pos = ignored + 1, pos + size
                    continue
                if not bos and (not self.links or self.bad or self.eos or serial != self.serial):
                    self.passed()
                    ignored, pos = ignored + 1, pos + size
                    continue
                disc = cont if bos else (seq != self.seq or cont != (self.open is not None))
                if (bos or disc) and took or taken == len(chunk) // 27 + 1:    # the most pages a call takes
                    stopped = True
                    break
                took, pos = True, pos + size
                self.passed()
                if bos:
                    self.links.append(Link())
                    self.serial, self.open, self.npk = serial, None, 0
                    self.bad = self.eos = False
                    self.gap = len(self.links) > 1
                    started = True
                    self.link_started()
                if disc:
                    if self.npk < 3:
                        self.bad = True
                        continue
                    self.open, self.gap = None, True
                self.page_taken(serial)
                body = page[27 + nseg:]
                if disc and cont:                    # the leading segments belong to no packet
                    while lacing:
                        lv = lacing.pop(0)
                        body = body[lv:]
                        if lv < 255:
                            break
                self.seq = (seq + 1) & 0xffffffff
                taken += 1
                completed = []
                for lv in lacing:
                    if self.open is None:
                        self.open = bytearray()
                    self.open += body[:lv]
                    body = body[lv:]
                    if lv < 255:
                        completed.append(bytes(self.open))
                        self.open = None
                link = self.links[-1]
                for k, pk in enumerate(completed):
                    last = k == len(completed) - 1
                    if self.npk < 3:
                        link.headers.append(pk)
                    else:
                        rec = (pk, granule if last else -1, int(bool(flags & 4) and last), int(self.gap))
                        self.gap = False
                        out.append(rec)
                        link.packets.append(rec[0]), link.granulepos.append(rec[1])
                        link.eos.append(rec[2]), link.gap.append(rec[3])
                    self.npk += 1
                if flags & 4:
                    self.eos = True
            if stopped:
                self.tail = run[pos:carried] if pos < carried else b""
                left = len(run) - max(pos, carried)
            else:
                self.tail = run[pos:]
            if end and not stopped:
                skipped += len(self.tail)
                self.tail, self.open, self.done = b"", None, True
        return {"packets": out, "link": max(len(self.links) - 1, 0), "link_started": int(started), "link_bad": int(self.bad),
                "gaps": sum(r[3] for r in out), "skipped": skipped, "ignored": ignored, "left": left,
                "headers_ready": int(bool(self.links) and self.npk >= 3 and not self.bad)}


def run(data, cuts=(), end=True, slot=None):
    """data cut at `cuts` (sorted positions), one call per piece and one more for every part a call leaves; `end` goes
    with the last piece.  -> (slot, [call records])"""
    slot = slot or Slot()
    edges = [0] + list(cuts) + [len(data)]
    calls = []
    for k in range(len(edges) - 1):
        chunk, last = bytes(data[edges[k]:edges[k + 1]]), end and k == len(edges) - 2
        while True:
            c = slot.call(chunk, last)
            calls.append(c)
            if not c["left"] and not (last and slot.tail):
                break
            chunk = chunk[len(chunk) - c["left"]:]
    return slot, calls
