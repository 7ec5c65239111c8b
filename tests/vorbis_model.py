"""An independent Vorbis I audio-packet decoder, a header writer, a packet writer and a seeded generator of valid but
unusual setups, for the decoder tests (test_decoder_model_cpu.py, test_decoder_synthetic_gpu.py; the corpus rows both
share are decode_packets.family).

The decoder is written from the specification in the reference tree (doc/Vorbis_I_spec.tex with 03-codebook.tex,
07-floor1.tex, 08-residue.tex), one bit at a time and one spec step at a time.  It shares no table layout with the
product's unpack: Huffman words are assigned by the spec's rule ("the lowest valued unused codeword of that length")
into a binary tree that is walked bit by bit; residue 2 is decoded as one residue-1 vector of ch*n and de-interleaved;
the floor curve is the spec's integer render_line loop.

Where the specification leaves room, or the reference decoder deviates from it, the model does what the reference
does (file:line in the reference tree):

  * end of packet inside a floor (flag, class word or Y word) marks the channel unused (lib/floor1.c:985-1017, the
    eop label; spec 7.2.3 says the same).  One place goes the other way: the reference does not test the reads of
    the two amplitude values (lib/floor1.c:988-989), so a floor with no book to read after them carries on with
    Y = -1.  There the model follows the specification (channel unused), and so does the product; the PCM is the
    same, since nothing of the packet is left for the residue
  * end of packet inside the residue keeps what was decoded: formats 1 and 2 keep the entries already added
    (lib/codebook.c:551-565, :593-), format 0 adds nothing of a partition whose entries are not all present
    (lib/codebook.c:531-548 decodes all of them before it adds any)
  * a class word whose value is >= classifications^dim ends the residue decode (lib/res0.c:677, :829); the spec
    would drop its high digits
  * a vector whose dimension does not divide the partition size is cut at the partition's end in formats 1 and 2
    (lib/codebook.c:560, :619: `i<n`, `i<m`); the spec's loop would run over it.  Format 0 reads n/dim entries and
    leaves the remainder untouched (lib/codebook.c:533)
  * unwrapped floor Y values are kept modulo 2^15 (lib/floor1.c:1046 `&0x7fff`) and clamped to [0, 255] after the
    multiplier (lib/floor1.c:1078, :1088); the spec has neither
  * a single-entry book of length 1 consumes one bit of either value (lib/sharedbook.c, vorbis_book_init_decode:
    the whole first-level table points at the entry); the spec calls a single-entry book's word length 1 as well
  * the packet status comes from the head bits alone (lib/synthesis.c:25-91): type bit -> ENOTAUDIO, mode (or
    the long block's lW / nW bits) missing or mode out of range -> EBADPACKET; nothing after them fails a packet
  * dequantised values: |q| * delta + min + last in double precision, rounded once to float32 per value
    (lib/sharedbook.c:243-268)
  * the residue-2 reference walks channels from 0 at every partition (lib/codebook.c:593-), which equals the spec's
    de-interleave only when `begin` and the partition size are multiples of the channel count: the generator keeps
    them so

Nothing here imports the product; the tests do the comparing."""
import math

import numpy as np

ENOTAUDIO, EBADPACKET = -135, -136
PAIRS = [(a, b) for a in (256, 512, 1024, 2048, 4096) for b in (256, 512, 1024, 2048, 4096) if a <= b]


def ilog(v):
    return int(v).bit_length()


# ---- bits ----------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSb first (spec 2.1.4)"""

    def __init__(self):
        self.bits = []

    def write(self, value, n):
        assert 0 <= value < (1 << n) or n == 0, (value, n)
        self.bits.extend((value >> i) & 1 for i in range(n))

    def write_code(self, code):
        """a Huffman word given as its bit string in reading order"""
        self.bits.extend(code)

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return np.packbits(np.array(b, np.uint8), bitorder="little").tobytes() if b else b""


class EndOfPacket(Exception):
    pass


class Bits:
    """reader; after a read that does not fit, every later read fails too"""

    def __init__(self, data):
        self.b = np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little").tolist()
        self.n, self.pos = len(self.b), 0

    def read(self, k):
        if self.pos + k > self.n:
            self.pos = self.n + 1
            raise EndOfPacket
        v = 0
        for i in range(k):
            v |= self.b[self.pos + i] << i
        self.pos += k
        return v


# ---- codebooks -------------------------------------------------------------------------------------------------------
def float32_unpack(x):
    """spec 9.2.2: 21-bit mantissa, 10-bit exponent biased by 788, sign"""
    mant = x & 0x1fffff
    if x & 0x80000000:
        mant = -mant
    return math.ldexp(mant, ((x & 0x7fe00000) >> 21) - 788)


def float32_pack(mant, exp):
    """inverse, for the generator: value mant * 2^exp"""
    assert abs(mant) < (1 << 21) and 0 <= exp + 788 < 1024
    return (0x80000000 if mant < 0 else 0) | ((exp + 788) << 21) | abs(mant)


def lookup1_values(entries, dim):
    """spec 9.2.3: the greatest integer v with v^dim <= entries, by integer search"""
    v = 0
    while (v + 1) ** dim <= entries:
        v += 1
    return v


class _Node:
    __slots__ = ("kid", "full")

    def __init__(self):
        self.kid, self.full = [None, None], False


def _place(node, length, entry):
    """put `entry` at the leftmost free leaf `length` below node (spec 3.2.1: lowest valued unused codeword of that
    length) -> its bits, or None if there is no room"""
    for bit in (0, 1):
        kid = node.kid[bit]
        if length == 1:
            if kid is None:
                node.kid[bit] = entry
                got = [bit]
            else:
                continue
        else:
            if kid is None:
                kid = node.kid[bit] = _Node()
            if not isinstance(kid, _Node) or kid.full:
                continue
            got = _place(kid, length - 1, entry)
            if got is None:
                continue
            got.insert(0, bit)
        node.full = all(k is not None and (not isinstance(k, _Node) or k.full) for k in node.kid)
        return got
    return None


class Book:
    def __init__(self, d):
        self.d = d
        self.dim, self.entries = d["dim"], d["entries"]
        self.used = [i for i, l in enumerate(d["lengthlist"]) if l > 0]
        self.single = len(self.used) == 1
        self.root, self.code = _Node(), {}
        if self.single:
            assert d["lengthlist"][self.used[0]] == 1
            self.code[self.used[0]] = [0]
        else:
            for i in self.used:
                self.code[i] = _place(self.root, d["lengthlist"][i], i)
                assert self.code[i] is not None, "overpopulated tree"
            assert self.root.full or not self.used, "underpopulated tree"
        self.maxlen = max(d["lengthlist"], default=0)
        self.vals = None
        if d["maptype"] in (1, 2):
            mn, delta = float32_unpack(d["q_min"]), float32_unpack(d["q_delta"])
            lv = lookup1_values(self.entries, self.dim) if d["maptype"] == 1 else 0
            self.vals = np.zeros((self.entries, self.dim), np.float32)
            for e in self.used:
                last, div = np.float32(0), 1
                for i in range(self.dim):
                    off = (e // div) % lv if d["maptype"] == 1 else e * self.dim + i
                    val = np.float32(float(d["quantlist"][off]) * delta + mn + float(last))
                    if d["q_sequencep"]:
                        last = val
                    self.vals[e, i] = val
                    div *= lv

    def decode(self, r, C):
        """scalar context -> entry number; EndOfPacket consumes the rest of the packet"""
        if not self.used:
            raise EndOfPacket
        if self.single:
            r.read(1)
            return self.used[0]
        node, bits, n, pos = self.root, r.b, r.n, r.pos
        start = pos
        while True:
            if pos >= n:
                r.pos = n + 1
                raise EndOfPacket
            node = node.kid[bits[pos]]
            pos += 1
            if not isinstance(node, _Node):
                break
        r.pos = pos
        if pos - start > 8:
            C["codeword_longer_than_8"] += 1
        if pos - start == 32:
            C["codeword_32_bits"] += 1
        return node


# ---- header writer: inverse of tests/decode_packets.unpack_headers ----------------------------------------------
def pack_book(w, b, coding="auto"):
    """coding: "ordered" (length runs), "dense" (5 bits per entry), "sparse" (flag + 5 bits), or "auto": what the
    reference's writer picks (ordered if the lengths never decrease and none is 0, else sparse if any is 0)"""
    L = b["lengthlist"]
    if coding == "auto":
        if all(l > 0 for l in L) and all(L[i] >= L[i - 1] for i in range(1, len(L))) and L:
            coding = "ordered"
        else:
            coding = "sparse" if any(l == 0 for l in L) else "dense"
    w.write(0x564342, 24)
    w.write(b["dim"], 16)
    w.write(b["entries"], 24)
    if coding == "ordered":
        assert all(l > 0 for l in L) and all(L[i] >= L[i - 1] for i in range(1, len(L)))
        w.write(1, 1)
        w.write(L[0] - 1, 5)
        done, length = 0, L[0]
        while done < len(L):
            num = sum(1 for l in L if l == length)
            w.write(num, ilog(len(L) - done))
            done += num
            length += 1
    else:
        w.write(0, 1)
        w.write(1 if coding == "sparse" else 0, 1)
        for l in L:
            if coding == "sparse":
                w.write(1 if l else 0, 1)
                if l:
                    w.write(l - 1, 5)
            else:
                assert l > 0
                w.write(l - 1, 5)
    w.write(b["maptype"], 4)
    if b["maptype"] in (1, 2):
        w.write(b["q_min"], 32)
        w.write(b["q_delta"], 32)
        w.write(b["q_quant"] - 1, 4)
        w.write(b["q_sequencep"], 1)
        for q in b["quantlist"]:
            w.write(q, b["q_quant"])


def pack_headers(s, coding=None, floor_types=None, framing=1):
    """setup dict (the layout unpack_headers returns) -> (identification, comment, setup) packets.  coding: per book,
    see pack_book.  floor_types / framing: for the rejected-setup tests."""
    w = BitWriter()
    w.write(1, 8)
    for c in b"vorbis":
        w.write(c, 8)
    w.write(0, 32)
    w.write(s["channels"], 8)
    w.write(s["rate"], 32)
    for x in s["bitrates"]:
        w.write(x & 0xffffffff, 32)
    w.write(ilog(s["blocksizes"][0] - 1), 4)
    w.write(ilog(s["blocksizes"][1] - 1), 4)
    w.write(1, 1)
    h0 = w.tobytes()

    w = BitWriter()
    w.write(3, 8)
    for c in b"vorbis":
        w.write(c, 8)
    w.write(len(s["vendor"]), 32)
    for c in s["vendor"]:
        w.write(c, 8)
    w.write(len(s["comments"]), 32)
    for cm in s["comments"]:
        w.write(len(cm), 32)
        for c in cm:
            w.write(c, 8)
    w.write(1, 1)
    h1 = w.tobytes()

    w = BitWriter()
    w.write(5, 8)
    for c in b"vorbis":
        w.write(c, 8)
    w.write(len(s["books"]) - 1, 8)
    for i, b in enumerate(s["books"]):
        pack_book(w, b, coding[i] if coding else "auto")
    w.write(0, 6)                               # one time-domain placeholder
    w.write(0, 16)
    w.write(len(s["floors"]) - 1, 6)
    for i, f in enumerate(s["floors"]):
        w.write(floor_types[i] if floor_types else 1, 16)
        w.write(f["partitions"], 5)
        for c in f["partitionclass"]:
            w.write(c, 4)
        for c in range(len(f["class_dim"])):
            w.write(f["class_dim"][c] - 1, 3)
            w.write(f["class_subs"][c], 2)
            if f["class_subs"][c]:
                w.write(f["class_book"][c], 8)
            for sb in f["class_subbook"][c]:
                w.write(sb + 1, 8)
        w.write(f["mult"] - 1, 2)
        rangebits = ilog(f["postlist"][1] - 1)
        assert f["postlist"][1] == 1 << rangebits
        w.write(rangebits, 4)
        for x in f["postlist"][2:]:
            w.write(x, rangebits)
    w.write(len(s["residues"]) - 1, 6)
    for r in s["residues"]:
        w.write(r["type"], 16)
        w.write(r["begin"], 24)
        w.write(r["end"], 24)
        w.write(r["grouping"] - 1, 24)
        w.write(r["partitions"] - 1, 6)
        w.write(r["groupbook"], 8)
        for c in r["secondstages"]:
            w.write(c & 7, 3)
            if c >> 3:
                w.write(1, 1)
                w.write(c >> 3, 5)
            else:
                w.write(0, 1)
        for b in r["booklist"]:
            w.write(b, 8)
    w.write(len(s["maps"]) - 1, 6)
    ch = s["channels"]
    for m in s["maps"]:
        w.write(0, 16)
        if m["submaps"] > 1:
            w.write(1, 1)
            w.write(m["submaps"] - 1, 4)
        else:
            w.write(0, 1)
        if m["coupling"]:
            w.write(1, 1)
            w.write(len(m["coupling"]) - 1, 8)
            for mag, ang in m["coupling"]:
                w.write(mag, ilog(ch - 1))
                w.write(ang, ilog(ch - 1))
        else:
            w.write(0, 1)
        w.write(0, 2)
        if m["submaps"] > 1:
            for x in m["chmuxlist"]:
                w.write(x, 4)
        for k in range(m["submaps"]):
            w.write(0, 8)
            w.write(m["floorsubmap"][k], 8)
            w.write(m["residuesubmap"][k], 8)
    w.write(len(s["modes"]) - 1, 6)
    for flag, wt, tt, mp in s["modes"]:
        w.write(flag, 1)
        w.write(wt, 16)
        w.write(tt, 16)
        w.write(mp, 8)
    w.write(framing, 1)
    return h0, h1, w.tobytes()


# ---- the decoder -----------------------------------------------------------------------------------------------------
COUNTERS = [
    "eop_floor_flag", "eop_floor_y", "eop_floor_class",
    "eop_classword_0", "eop_classword_1", "eop_classword_2", "eop_residue_0", "eop_residue_1", "eop_residue_2",
    "codeword_longer_than_8", "codeword_32_bits", "y_clamped", "floor_room_tie_unwrapped",
    "post_at_or_above_n", "classword_out_of_range",
    "empty_residue_range", "unused_subbook_zero", "floor_wrapped", "floor_unwrapped", "floor_predicted",
    "couple_m_pos_a_pos", "couple_m_pos_a_neg", "couple_m_neg_a_pos", "couple_m_neg_a_neg",
    "format0_partial_partition_dropped", "vector_cut_at_partition_end", "single_entry_book_read",
    "enotaudio", "ebadpacket_mode", "ebadpacket_eop",
]


def render_point(x0, y0, x1, y1, x):
    dy, adx = y1 - y0, x1 - x0
    off = abs(dy) * (x - x0) // adx
    return y0 - off if dy < 0 else y0 + off


def render_line(x0, y0, x1, y1, v, n):
    """spec 9.2.7, writing only the bins below n"""
    dy, adx = y1 - y0, x1 - x0
    ady = abs(dy)
    base = -(ady // adx) if dy < 0 else ady // adx          # dy / adx rounded toward zero
    sy = base - 1 if dy < 0 else base + 1
    ady -= abs(base) * adx
    x, y, err = x0, y0, 0
    if x < n:
        v[x] = y
    for x in range(x0 + 1, min(x1, n)):
        err += ady
        if err >= adx:
            err -= adx
            y += sy
        else:
            y += base
        v[x] = y


class Model:
    def __init__(self, setup, fromdB):
        self.s = setup
        self.fromdB = np.asarray(fromdB, np.float32)
        self.books = [Book(b) for b in setup["books"]]
        self.ch, self.bs = setup["channels"], setup["blocksizes"]
        self.modebits = ilog(len(setup["modes"]) - 1)
        self.C = {k: 0 for k in COUNTERS}

    # -- floor 1 (spec 7.2.3, 7.2.4) --
    def floor_read(self, f, r):
        """-> the Y list, or None: unused"""
        C = self.C
        try:
            if r.read(1) == 0:
                return None
        except EndOfPacket:
            C["eop_floor_flag"] += 1
            return None
        rng = (256, 128, 86, 64)[f["mult"] - 1]
        try:
            Y = [r.read(ilog(rng - 1)), r.read(ilog(rng - 1))]
        except EndOfPacket:
            C["eop_floor_y"] += 1
            return None
        for cls in f["partitionclass"]:
            cdim, cbits = f["class_dim"][cls], f["class_subs"][cls]
            cval = 0
            if cbits:
                try:
                    cval = self.books[f["class_book"][cls]].decode(r, C)
                except EndOfPacket:
                    C["eop_floor_class"] += 1
                    return None
            for _ in range(cdim):
                book = f["class_subbook"][cls][cval & ((1 << cbits) - 1)]
                cval >>= cbits
                if book >= 0:
                    try:
                        Y.append(self.books[book].decode(r, C))
                    except EndOfPacket:
                        C["eop_floor_y"] += 1
                        return None
                else:
                    C["unused_subbook_zero"] += 1
                    Y.append(0)
        return Y

    def floor_curve(self, f, Y, n):
        """-> the index into the dB table per bin [n]"""
        C = self.C
        X = f["postlist"]
        rng = (256, 128, 86, 64)[f["mult"] - 1]
        final, flag = [Y[0], Y[1]], [True, True]
        for i in range(2, len(X)):
            lo = max((j for j in range(i) if X[j] < X[i]), key=lambda j: X[j])
            hi = min((j for j in range(i) if X[j] > X[i]), key=lambda j: X[j])
            pred = render_point(X[lo], final[lo], X[hi], final[hi], X[i])
            val, highroom, lowroom = Y[i], rng - pred, pred
            room = 2 * min(highroom, lowroom)
            if val:
                flag[lo] = flag[hi] = True
                flag.append(True)
                if val >= room:
                    C["floor_unwrapped"] += 1
                    if highroom == lowroom:
                        C["floor_room_tie_unwrapped"] += 1
                    fy = val - lowroom + pred if highroom > lowroom else pred - val + highroom - 1
                else:
                    C["floor_wrapped"] += 1
                    fy = pred - (val + 1) // 2 if val & 1 else pred + val // 2
                final.append(fy & 0x7fff)
            else:
                C["floor_predicted"] += 1
                flag.append(False)
                final.append(pred)
        order = sorted(range(len(X)), key=lambda j: X[j])

        def scaled(j):
            y = final[j] * f["mult"]
            if y > 255 or y < 0:
                C["y_clamped"] += 1
            return min(max(y, 0), 255)

        v = [0] * n
        hx, lx, ly = 0, 0, scaled(order[0])
        hy = ly
        for j in order[1:]:
            if flag[j]:
                hy, hx = scaled(j), X[j]
                if hx >= n:
                    C["post_at_or_above_n"] += 1
                render_line(lx, ly, hx, hy, v, n)
                lx, ly = hx, hy
        for x in range(hx, n):
            v[x] = hy
        return np.array(v, np.int32)

    # -- residue (spec 8.6.2 - 8.6.5) --
    def residue_decode(self, res, r, nvec, size, skip):
        """nvec vectors of `size` values, format 0 or 1 layout -> float32 [nvec][size].  skip[j]: do not decode"""
        C = self.C
        t = res["type"]
        fmt = 0 if t == 0 else 1
        out = np.zeros((nvec, size), np.float32)
        begin, end = min(res["begin"], size), min(res["end"], size)
        psize = res["grouping"]
        nclass = res["partitions"]
        gbook = self.books[res["groupbook"]]
        cpw = gbook.dim
        n_to_read = end - begin
        if res["end"] <= res["begin"] or res["begin"] >= size or n_to_read <= 0:
            C["empty_residue_range"] += 1
            return out
        nparts = n_to_read // psize
        # the stage books of each class, in header order
        stage = [[-1] * 8 for _ in range(nclass)]
        it = iter(res["booklist"])
        for c in range(nclass):
            for st in range(8):
                if res["secondstages"][c] >> st & 1:
                    stage[c][st] = next(it)
        cls = [[0] * (nparts + cpw) for _ in range(nvec)]
        for st in range(8):
            pc = 0
            while pc < nparts:
                if st == 0:
                    for j in range(nvec):
                        if skip[j]:
                            continue
                        try:
                            temp = gbook.decode(r, C)
                        except EndOfPacket:
                            C[f"eop_classword_{t}"] += 1
                            return out
                        if temp >= nclass ** cpw:
                            C["classword_out_of_range"] += 1
                            return out
                        for i in range(cpw - 1, -1, -1):
                            cls[j][i + pc] = temp % nclass
                            temp //= nclass
                for _ in range(cpw):
                    if pc >= nparts:
                        break
                    for j in range(nvec):
                        if skip[j]:
                            continue
                        bk = stage[cls[j][pc]][st]
                        if bk < 0:
                            continue
                        book = self.books[bk]
                        off = begin + pc * psize
                        try:
                            if fmt == 0:
                                step = psize // book.dim
                                got = []
                                try:
                                    for _k in range(step):
                                        got.append(book.decode(r, C))
                                except EndOfPacket:
                                    if got:
                                        C["format0_partial_partition_dropped"] += 1
                                    raise
                                for i, e in enumerate(got):
                                    out[j, off + i:off + i + book.dim * step:step] += book.vals[e]
                            else:
                                i = 0
                                while i < psize:
                                    e = book.decode(r, C)
                                    k = min(book.dim, psize - i)
                                    if k < book.dim:
                                        C["vector_cut_at_partition_end"] += 1
                                    out[j, off + i:off + i + k] += book.vals[e, :k]
                                    i += book.dim
                        except EndOfPacket:
                            C[f"eop_residue_{t}"] += 1
                            return out
                    pc += 1
        return out

    # -- one audio packet (spec 4.3) --
    def decode(self, pkt):
        C, s, ch = self.C, self.s, self.ch
        half = self.bs[1] // 2
        out = {"status": 0, "info": [0, 0, 0, 0], "used_before": np.zeros(ch, np.int32),
               "used": np.zeros(ch, np.int32), "floor_index": np.zeros((ch, half), np.int32),
               "residue": np.zeros((ch, half), np.float32), "spectrum": np.zeros((ch, half), np.float32)}
        r = Bits(pkt)
        try:
            if r.read(1) != 0:
                raise EndOfPacket
        except EndOfPacket:
            C["enotaudio"] += 1
            out["status"] = ENOTAUDIO
            return out
        try:
            mode = r.read(self.modebits)
            if mode >= len(s["modes"]):
                C["ebadpacket_mode"] += 1
                out["status"] = EBADPACKET
                return out
            W = s["modes"][mode][0]
            lW = nW = 0
            if W:
                lW, nW = r.read(1), r.read(1)
        except EndOfPacket:
            C["ebadpacket_eop"] += 1
            out["status"] = EBADPACKET
            return out
        out["info"] = [mode, W, lW, nW]
        m = s["maps"][s["modes"][mode][3]]
        n = self.bs[W] // 2
        floors = []
        for c in range(ch):
            f = s["floors"][m["floorsubmap"][m["chmuxlist"][c]]]
            Y = self.floor_read(f, r)
            floors.append((f, Y))
            if Y is not None:
                out["used_before"][c] = 1
                out["floor_index"][c, :n] = self.floor_curve(f, Y, n)
        used = [int(Y is not None) for _, Y in floors]
        for mag, ang in m["coupling"]:
            if used[mag] or used[ang]:
                used[mag] = used[ang] = 1
        out["used"][:] = used
        resid = np.zeros((ch, n), np.float32)
        for sm in range(m["submaps"]):
            chans = [c for c in range(ch) if m["chmuxlist"][c] == sm]
            res = s["residues"][m["residuesubmap"][sm]]
            if not chans:
                continue
            if res["type"] == 2:
                if not any(used[c] for c in chans):
                    continue
                vec = self.residue_decode(res, r, 1, n * len(chans), [False])[0]
                for i, c in enumerate(chans):
                    resid[c] = vec[i::len(chans)]
            else:
                # unused channels are not decoded; the reference compacts them away
                live = [c for c in chans if used[c]]
                if not live:
                    continue
                vec = self.residue_decode(res, r, len(live), n, [False] * len(live))
                for i, c in enumerate(live):
                    resid[c] = vec[i]
        out["residue"][:, :n] = resid
        v = resid.copy()
        for mag, ang in reversed(m["coupling"]):
            M, A = v[mag].copy(), v[ang].copy()
            pp, pn, np_, nn = (M > 0) & (A > 0), (M > 0) & ~(A > 0), ~(M > 0) & (A > 0), ~(M > 0) & ~(A > 0)
            C["couple_m_pos_a_pos"] += int(pp.sum())
            C["couple_m_pos_a_neg"] += int((pn & (A < 0)).sum())
            C["couple_m_neg_a_pos"] += int((np_ & (M < 0)).sum())
            C["couple_m_neg_a_neg"] += int((nn & (M < 0) & (A < 0)).sum())
            newM = np.where(pp, M, np.where(pn, M + A, np.where(np_, M, M - A))).astype(np.float32)
            newA = np.where(pp, M - A, np.where(pn, M, np.where(np_, M + A, M))).astype(np.float32)
            v[mag], v[ang] = newM, newA
        for c in range(ch):
            if out["used_before"][c]:
                out["spectrum"][c, :n] = v[c] * self.fromdB[out["floor_index"][c, :n]]
        return out


# ---- packet writer ---------------------------------------------------------------------------------------------------
class PacketWriter:
    """Builds an audio packet field by field with chosen content, following the same packet layout (spec 4.3) the
    decoder reads; it needs no decoding to know what it wrote."""

    def __init__(self, model, rng):
        self.m, self.rng = model, rng

    def _entry(self, book):
        return book.used[int(self.rng.integers(len(book.used)))]

    def _put(self, w, book, e):
        w.write_code(book.code[e])
        if book.single:
            self.m.C["single_entry_book_read"] += 1

    def packet(self, mode, lW=None, nW=None, p_floor=0.85, loud=False, bad_classword=0.0, tie=False):
        """loud: every floor used with high end values (for the PCM streams).  tie: both end values at half the
        range and every post either predicted or coded with a value >= the range, so that posts are unwrapped where
        the room above and below the prediction is equal"""
        mdl, s, rng = self.m, self.m.s, self.rng
        w = BitWriter()
        w.write(0, 1)
        w.write(mode, mdl.modebits)
        W = s["modes"][mode][0]
        if W:
            w.write(int(rng.integers(2)) if lW is None else lW, 1)
            w.write(int(rng.integers(2)) if nW is None else nW, 1)
        m = s["maps"][s["modes"][mode][3]]
        n = mdl.bs[W] // 2
        ch = mdl.ch
        used = []
        for c in range(ch):
            f = s["floors"][m["floorsubmap"][m["chmuxlist"][c]]]
            u = loud or tie or rng.random() < p_floor
            used.append(int(u))
            w.write(int(u), 1)
            if not u:
                continue
            rngv = (256, 128, 86, 64)[f["mult"] - 1]
            qb = ilog(rngv - 1)
            for _ in range(2):
                w.write(rngv // 2 if tie else int(rng.integers(int(0.7 * rngv), rngv)) if loud
                        else int(rng.integers(1 << qb)), qb)
            for cls in f["partitionclass"]:
                cbits = f["class_subs"][cls]
                cval = 0
                if cbits:
                    bk = mdl.books[f["class_book"][cls]]
                    cval = self._entry(bk)
                    self._put(w, bk, cval)
                for _ in range(f["class_dim"][cls]):
                    book = f["class_subbook"][cls][cval & ((1 << cbits) - 1)]
                    cval >>= cbits
                    if book >= 0:
                        bk = mdl.books[book]
                        # mostly small codes (near the prediction), sometimes any
                        e = self._entry(bk)
                        if rng.random() < 0.6:
                            e = bk.used[int(rng.integers(min(4, len(bk.used))))]
                        if tie:
                            big = [x for x in bk.used if x >= rngv]
                            e = big[int(rng.integers(len(big)))] if big and rng.random() < 0.3 else bk.used[0]
                        self._put(w, bk, e)
        for mag, ang in m["coupling"]:
            if used[mag] or used[ang]:
                used[mag] = used[ang] = 1
        for sm in range(m["submaps"]):
            chans = [c for c in range(ch) if m["chmuxlist"][c] == sm]
            res = s["residues"][m["residuesubmap"][sm]]
            if not chans:
                continue
            if res["type"] == 2:
                if not any(used[c] for c in chans):
                    continue
                nvec, size = 1, n * len(chans)
            else:
                nvec, size = sum(used[c] for c in chans), n
                if not nvec:
                    continue
            if not self._residue(w, res, nvec, size, bad_classword):
                break
        return w.tobytes()

    def _residue(self, w, res, nvec, size, bad_classword):
        mdl, rng = self.m, self.rng
        begin, end = min(res["begin"], size), min(res["end"], size)
        if end - begin <= 0:
            return True
        psize, nclass = res["grouping"], res["partitions"]
        nparts = (end - begin) // psize
        gbook = mdl.books[res["groupbook"]]
        cpw = gbook.dim
        stage = [[-1] * 8 for _ in range(nclass)]
        it = iter(res["booklist"])
        for c in range(nclass):
            for st in range(8):
                if res["secondstages"][c] >> st & 1:
                    stage[c][st] = next(it)
        good = [e for e in gbook.used if e < nclass ** cpw]
        bad = [e for e in gbook.used if e >= nclass ** cpw]
        cls = [[0] * (nparts + cpw) for _ in range(nvec)]
        for st in range(8):
            pc = 0
            while pc < nparts:
                if st == 0:
                    for j in range(nvec):
                        if bad and rng.random() < bad_classword:
                            self._put(w, gbook, bad[int(rng.integers(len(bad)))])
                            return False
                        if not good:
                            return False
                        temp = good[int(rng.integers(len(good)))]
                        self._put(w, gbook, temp)
                        for i in range(cpw - 1, -1, -1):
                            cls[j][i + pc] = temp % nclass
                            temp //= nclass
                for _ in range(cpw):
                    if pc >= nparts:
                        break
                    for j in range(nvec):
                        bk = stage[cls[j][pc]][st]
                        if bk < 0:
                            continue
                        book = mdl.books[bk]
                        count = psize // book.dim if res["type"] == 0 else -(-psize // book.dim)
                        for _k in range(count):
                            self._put(w, book, self._entry(book))
                    pc += 1
        return True


# ---- setup generator -------------------------------------------------------------------------------------------------
def make_lengths(rng, used, maxlen):
    """`used` codeword lengths of a complete tree (Kraft sum exactly 1) whose longest word has maxlen bits"""
    assert used >= 2
    deep = min(maxlen, used - 1, 32)
    L = list(range(1, deep)) + [deep, deep]
    while len(L) < used:
        cand = [i for i, l in enumerate(L) if l < deep]
        if not cand:
            deep = min(deep + 1, 32)
            cand = [i for i, l in enumerate(L) if l < deep]
        i = cand[int(rng.integers(len(cand)))]
        L[i] += 1
        L.append(L[i])
    assert sum(2.0 ** -l for l in L) == 1.0
    return L


class _Gen:
    def __init__(self, rng, min_exp):
        self.rng, self.books, self.coding, self.min_exp = rng, [], [], min_exp

    def add(self, book, coding):
        self.books.append(book)
        self.coding.append(coding)
        return len(self.books) - 1

    def lengths(self, entries, maxlen, style):
        """style: "ordered", "dense", "sparse" (unused entries between used ones), "single" """
        rng = self.rng
        if style == "single":
            L = [0] * entries
            L[int(rng.integers(entries))] = 1
            return L, "sparse"
        if style == "sparse":
            used = max(2, entries - max(1, entries // 4))
            L = make_lengths(rng, used, maxlen)
            rng.shuffle(L)
            holes = set(rng.choice(np.arange(1, entries - 1), entries - used, replace=False).tolist()) \
                if entries > used else set()
            out, it = [], iter(L)
            for i in range(entries):
                out.append(0 if i in holes else next(it))
            return out, "sparse"
        L = make_lengths(rng, entries, maxlen)
        if style == "ordered":
            return sorted(L), "ordered"
        rng.shuffle(L)
        return [int(x) for x in L], ("dense" if style == "dense" else "sparse")

    def scalar_book(self, entries, maxlen=10, style="dense"):
        L, coding = self.lengths(entries, maxlen, style)
        return self.add({"dim": int(self.rng.integers(1, 3)), "entries": entries, "lengthlist": [int(x) for x in L],
                         "maptype": 0}, coding)

    def value_book(self, dim, maptype=1, seq=0, maxlen=10, style="dense", entries=None, inexact=False):
        rng = self.rng
        if maptype == 1:
            lv = int(rng.integers(2, 5)) if dim <= 3 else (int(rng.integers(2, 4)) if dim <= 5 else 2)
            if dim == 1:
                lv = int(rng.integers(2, 17))
            entries = lv ** dim + (int(rng.integers(0, 3)) if style != "single" and dim > 1 else 0)
            assert lookup1_values(entries, dim) == lv
            nq = lv
        else:
            entries = entries or int(rng.integers(3, 40))
            nq = entries * dim
        L, coding = self.lengths(entries, maxlen, style)
        q_quant = int(rng.integers(2, 6))
        mid = 1 << (q_quant - 1)
        mant = int(rng.integers(1 << 12, 1 << 16)) | 1 if inexact else int(rng.choice([1, 3, 5]))
        exp = int(rng.integers(self.min_exp, self.min_exp + 8))
        book = {"dim": dim, "entries": entries, "lengthlist": [int(x) for x in L], "maptype": maptype,
                "q_min": float32_pack(-mant * (0 if seq else mid), exp), "q_delta": float32_pack(mant, exp),
                "q_quant": q_quant, "q_sequencep": seq,
                "quantlist": [int(x) for x in rng.integers(0, 1 << q_quant, nq)]}
        if seq:                          # running sums: centre them with a negative first step
            book["q_min"] = float32_pack(-mant * (mid // 2), exp)
        return self.add(book, coding)


def gen_setup(seed, ch=2, bs=(256, 2048), nmodes=2, res_types=(1,), submaps=1, coupling="none", mults=(2,),
              shared=False, maxlen=10, styles=("dense", "ordered", "sparse"), res_kw=None, maptypes=(1,), seq=(0,),
              group_dims=(2,), rangebits=None, min_exp=-10, inexact=False, stage_dims=(1, 2, 4), y_entries=(16, 40),
              single_books=False):
    """-> (setup dict, per-book header coding).  Every argument names one family of the corpus; see CORPUS."""
    rng = np.random.default_rng(seed)
    g = _Gen(rng, min_exp)
    res_kw = res_kw or {}
    pick = lambda seq_: seq_[int(rng.integers(len(seq_)))]           # noqa: E731
    nmaps = 1 if shared else min(nmodes, 2)
    floors, residues, maps = [], [], []

    def floor(n_block, mult):
        nclass = int(rng.integers(1, 4))
        cdim = [int(rng.integers(1, 6)) for _ in range(nclass)]
        csubs = [int(rng.integers(0, 4)) for _ in range(nclass)]
        csubs[0] = 0 if nclass > 1 else csubs[0]
        cbook, csb = [], []
        for c in range(nclass):
            cbook.append(g.scalar_book(int(rng.integers(2, 20)), maxlen=6, style=pick(styles)) if csubs[c] else None)
            sbs = []
            for k in range(1 << csubs[c]):
                if rng.random() < 0.25 or (c == 0 and nclass > 1 and k == 0):
                    sbs.append(-1)                               # unused sub-book: the Y value is 0
                elif single_books and rng.random() < 0.3:
                    sbs.append(g.scalar_book(int(rng.integers(2, 6)), style="single"))
                else:
                    sbs.append(g.scalar_book(int(rng.integers(*y_entries)), maxlen=maxlen, style=pick(styles)))
            csb.append(sbs)
        nparts = int(rng.integers(1, 7))
        pclass = [int(rng.integers(nclass)) for _ in range(nparts)]
        pclass[0] = nclass - 1                                  # the highest class is used: the header sends max + 1
        while sum(cdim[c] for c in pclass) > 40:
            pclass.pop()
        rb = rangebits or max(6, ilog(n_block - 1) + int(rng.integers(-1, 2)))
        count = sum(cdim[c] for c in pclass)
        xs = rng.choice(np.arange(1, 1 << rb), count, replace=False).tolist()
        return {"partitions": len(pclass), "partitionclass": pclass, "class_dim": cdim, "class_subs": csubs,
                "class_book": cbook, "class_subbook": csb, "mult": mult, "postlist": [0, 1 << rb] + [int(x) for x in xs]}

    def residue(rtype, n_block, nch):
        unit = nch if rtype == 2 else 1
        size = n_block * unit
        nclass = res_kw.get("classes") or int(rng.integers(2, 6))
        gdim = pick(group_dims)
        grouping = res_kw.get("grouping") or unit * int(pick([3, 4, 5, 6, 8, 16, 32]))
        begin = res_kw.get("begin", 0) * unit
        endk = res_kw.get("end", "at")
        end = {"at": size, "below": begin + (size - begin) // 2 // grouping * grouping + (grouping // 2),
               "above": size + 1000, "le_begin": begin, "huge": (1 << 24) - 1}[endk]
        extra = int(rng.integers(1, 4)) if res_kw.get("bad_classwords", True) else 0
        L, coding = g.lengths(nclass ** gdim + extra, maxlen=min(maxlen, 12), style=pick(styles))
        gb = g.add({"dim": gdim, "entries": len(L), "lengthlist": [int(x) for x in L], "maptype": 0}, coding)
        masks = res_kw.get("masks") or [0, 1, 2, 3, 5, 6, 7]
        stages = [int(pick(masks)) for _ in range(nclass)]
        stages[0] = 0                                           # a class with no books
        if nclass > 1:
            stages[1] = int(masks[-1])
        booklist = []
        for c in range(nclass):
            for st in range(8):
                if stages[c] >> st & 1:
                    sty = pick(styles)
                    if single_books and rng.random() < 0.25:
                        sty = "single"
                    booklist.append(g.value_book(int(pick(stage_dims)), maptype=pick(maptypes), seq=pick(seq),
                                                 maxlen=maxlen, style=sty, inexact=inexact))
        return {"type": rtype, "begin": begin, "end": end, "grouping": grouping, "partitions": nclass, "groupbook": gb,
                "secondstages": stages, "booklist": booklist}

    for mp in range(nmaps):
        n_block = bs[0] // 2 if (shared or mp == 0) else bs[1] // 2
        if shared:
            n_big = bs[1] // 2
        mux = [int(rng.integers(submaps)) for _ in range(ch)] if submaps > 1 else [0] * ch
        if submaps > 1:
            for k in range(min(submaps, ch)):
                mux[k] = k
        cp = []
        if ch > 1 and coupling != "none":
            if coupling == "pairs":
                cp = [(2 * k, 2 * k + 1) for k in range(ch // 2)]
            elif coupling == "chain":                           # channel 0 in every step, both roles
                cp = [(0, k) for k in range(1, ch)] + [(k, 0) for k in range(1, min(ch, 3))]
            else:
                for _ in range(int(rng.integers(1, 6))):
                    a, b = rng.choice(ch, 2, replace=False)
                    cp.append((int(a), int(b)))
        fsub, rsub = [], []
        for sm in range(submaps):
            nch = sum(1 for x in mux if x == sm)
            floors.append(floor(n_big if shared else n_block, pick(mults) if len(floors) >= len(mults) else mults[len(floors)]))
            fsub.append(len(floors) - 1)
            rt = res_types[len(residues) % len(res_types)]
            residues.append(residue(rt, n_block, max(nch, 1)))
            rsub.append(len(residues) - 1)
        maps.append({"submaps": submaps, "coupling": cp, "chmuxlist": mux, "floorsubmap": fsub, "residuesubmap": rsub})
    modes = []
    for i in range(nmodes):
        flag = i % 2 if nmodes > 1 else 0
        modes.append((flag, 0, 0, 0 if shared else min(flag, nmaps - 1)))
    setup = {"channels": ch, "rate": 44100, "bitrates": [0, 0, 0], "blocksizes": list(bs), "vendor": b"model",
             "comments": [b"SEED=%d" % seed], "books": g.books, "floors": floors, "residues": residues, "maps": maps,
             "modes": modes}
    assert len(g.books) <= 256
    return setup, g.coding


# One entry per family: (name, gen_setup arguments).  The first 15 cover the 15 block-size pairs.  The coverage test
# names the family to look at when one of its features goes missing.
CORPUS = [
    ("pair_256_256_grouping1",
     dict(ch=3, bs=PAIRS[0], res_types=(1,), res_kw=dict(grouping=1), stage_dims=(1,), nmodes=2, shared=True)),
    ("pair_256_512_res0", dict(ch=2, bs=PAIRS[1], res_types=(0,), coupling="pairs", stage_dims=(1, 2, 3, 4))),
    ("pair_256_1024_res2_odd_dims", dict(ch=3, bs=PAIRS[2], res_types=(2,), stage_dims=(2, 4, 5), coupling="random")),
    ("pair_256_2048_maptype2",
     dict(ch=2, bs=PAIRS[3], res_types=(1, 2), maptypes=(2,), coupling="pairs", inexact=True)),
    ("pair_256_4096_shared_floor", dict(ch=1, bs=PAIRS[4], shared=True, rangebits=10, res_kw=dict(end="huge"))),
    ("pair_512_512_mult1_mult3",
     dict(ch=4, bs=PAIRS[5], mults=(1, 3), y_entries=(100, 200), coupling="chain", res_types=(2, 0))),
    ("pair_512_1024_submaps",
     dict(ch=8, bs=PAIRS[6], submaps=5, nmodes=3, res_types=(0, 1, 2), coupling="random", mults=(1, 2, 3, 4),
     y_entries=(66, 130))),
    ("pair_512_2048_begin_end",
     dict(ch=2, bs=PAIRS[7], res_types=(1, 0), res_kw=dict(begin=7, end="below"), coupling="pairs", nmodes=12)),
    ("pair_512_4096_long_codewords",
     dict(ch=1, bs=PAIRS[8], maxlen=32, styles=("dense", "ordered"), stage_dims=(4, 8))),
    ("pair_1024_1024_seq",
     dict(ch=5, bs=PAIRS[9], seq=(1,), maptypes=(1, 2), res_types=(1, 2), coupling="chain", nmodes=20)),
    ("pair_1024_2048_stages_5_8",
     dict(ch=2, bs=PAIRS[10], res_kw=dict(masks=[0, 5, 0b10100000, 0b11111111, 0b1000101]), coupling="pairs",
     res_types=(2, 1), inexact=True)),
    ("pair_1024_4096_group_dims",
     dict(ch=6, bs=PAIRS[11], group_dims=(1, 3, 4), res_kw=dict(grouping=None, classes=3), res_types=(1, 2, 0),
     coupling="pairs", submaps=2)),
    ("pair_2048_2048_end_le_begin", dict(ch=2, bs=PAIRS[12], res_kw=dict(begin=16, end="le_begin"), coupling="pairs")),
    ("pair_2048_4096_end_above",
     dict(ch=7, bs=PAIRS[13], res_kw=dict(begin=3, end="above"), res_types=(2, 1), coupling="random", submaps=3)),
    ("pair_4096_4096_single_books", dict(ch=2, bs=PAIRS[14], single_books=True, res_types=(0, 1), coupling="pairs")),
    ("modes_64", dict(ch=2, bs=(256, 2048), nmodes=64, res_types=(1,), coupling="pairs")),
    ("modes_1", dict(ch=2, bs=(512, 1024), nmodes=1, res_types=(2,))),
    ("modes_5_submaps_16",
     dict(ch=8, bs=(256, 512), nmodes=5, submaps=16, res_types=(1, 0), coupling="chain", res_kw=dict(masks=[0, 1,
     2], classes=2))),
    ("group_dim4_ragged",
     dict(ch=2, bs=(256, 512), group_dims=(4,), res_kw=dict(grouping=6, classes=3), res_types=(1, 0),
     coupling="pairs")),
    ("sparse_32bit",
     dict(ch=2, bs=(256, 1024), maxlen=32, styles=("sparse",), res_types=(2,), coupling="pairs", maptypes=(1, 2))),
]


def build_corpus_setup(k):
    name, kw = CORPUS[k]
    return gen_setup(1000 + k, **kw)


def corpus_packets(model, headers, seed, nwriter=6):
    """-> [(label, packet bytes)] of one setup: writer-made packets, truncations, garbage tails, random bytes, the
    empty packet, the headers, and a mode index past the last mode"""
    rng = np.random.default_rng(seed)
    pw = PacketWriter(model, rng)
    nm = len(model.s["modes"])
    modes = sorted({0, nm - 1, nm // 2, min(1, nm - 1)})
    made = []
    for i in range(nwriter):
        mode = modes[i % len(modes)]
        made.append(pw.packet(mode, p_floor=(0.9, 0.6, 1.0)[i % 3], bad_classword=0.02 if i % 3 == 1 else 0.0))
    made += [pw.packet(modes[i % len(modes)], tie=True) for i in range(2)]
    out = [(f"writer{i}", p) for i, p in enumerate(made)]
    for i, p in enumerate(made[:nwriter]):
        cuts = sorted({1, 2, 3, 5, 8, len(p) // 7, len(p) // 3, len(p) // 2, (2 * len(p)) // 3, len(p) - 2, len(p) - 1})
        out += [(f"writer{i}[:{c}]", p[:c]) for c in cuts if 0 < c < len(p)]
        out.append((f"writer{i}+garbage", p + rng.integers(0, 256, 24, dtype=np.uint8).tobytes()))
    for i in range(6):
        b = bytearray(rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes())
        if i % 2 == 0:
            b[0] &= 0xFE
            if i == 0:                                       # a valid mode, so that the random bits reach the floor
                b[0] &= ~(((1 << model.modebits) - 1) << 1) & 0xFF
        out.append((f"random{i}", bytes(b)))
    out.append(("empty", b""))
    out += [(f"header{i}", h) for i, h in enumerate(headers)]
    if nm < (1 << model.modebits):
        w = BitWriter()
        w.write(0, 1)
        w.write(nm, model.modebits)
        w.write(0x3FFFFFF, 30)
        out.append(("mode_past_last", w.tobytes()))
    return out


def check_scales(result):
    """every nonzero value of a decoded packet has magnitude in [2^-60, 2^40] (no denormals, no overflow)"""
    for k in ("residue", "spectrum"):
        a = np.abs(result[k].astype(np.float64))
        nz = a[a != 0]
        assert np.isfinite(a).all() and (nz.size == 0 or (nz.min() >= 2.0 ** -60 and nz.max() <= 2.0 ** 40)), k


# ---- streams for the PCM tests ---------------------------------------------------------------------------------------
SEQUENCES = ["SSLLSLSSLL", "LLSLSSLSLL", "SLLLSSSLSL"]      # each has short->short, short->long, long->short, long->long


def pcm_setup(k):
    """one setup per block-size pair whose writer-made packets are loud: values are 0 or >= 1 in magnitude"""
    ch = (2, 1, 3, 2, 7)[k % 5]
    return gen_setup(2000 + k, ch=ch, bs=PAIRS[k], res_types=((1,), (2,), (0,), (1, 2))[k % 4], min_exp=0,
                     coupling="pairs" if ch > 1 else "none", nmodes=2 + k % 2, inexact=bool(k % 2),
                     res_kw=dict(bad_classwords=False, masks=[1, 3, 5, 7]))


def pcm_streams(model, seed, sequences=SEQUENCES, trim=37):
    """-> per stream [(packet, granulepos, eos)]: writer-made loud packets following a block-size sequence; the second
    stream's lW / nW bits contradict its real neighbours; the last packet carries a granule position `trim` samples
    short of the stream's length, and the end-of-stream flag"""
    rng = np.random.default_rng(seed)
    pw = PacketWriter(model, rng)
    bs = model.bs
    by_flag = {f: [i for i, md in enumerate(model.s["modes"]) if md[0] == f] for f in (0, 1)}
    out = []
    for si, seq in enumerate(sequences):
        flags = [0 if c == "S" or not by_flag[1] else 1 for c in seq]
        pk, total = [], 0
        for t, f in enumerate(flags):
            real_l = flags[t - 1] if t else 0
            real_n = flags[t + 1] if t + 1 < len(flags) else 0
            lW, nW = (1 - real_l, 1 - real_n) if si == 1 else (real_l, real_n)
            mode = by_flag[f][int(rng.integers(len(by_flag[f])))]
            if t:
                total += bs[flags[t - 1]] // 4 + bs[f] // 4
            last = t == len(flags) - 1
            pk.append((pw.packet(mode, lW=lW, nW=nW, loud=True), total - trim if last else -1, int(last)))
        out.append(pk)
    return out


def vorbis_window64(n):
    """the Vorbis window's rising half for a block of 2n samples, in float64 (spec 4.3.1: sin(pi/2 sin^2(...)))"""
    x = (np.arange(n) + 0.5) / n * (np.pi / 2)
    return np.sin(np.pi / 2 * np.sin(x) ** 2)
