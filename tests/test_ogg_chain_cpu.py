"""The split of chained Ogg files into links on the host twin (vbm_host_ogg_chain_split, split_ogg_chain): link starts
equal to a page walker written from the rule (ogg_chain_cases.walk), every link demuxed as vbm_ogg_demux demuxes its bytes
alone, and the consequences of the rule that DESIGN.md §9f lists.  Host only: runs without a GPU."""
import ctypes as C
import mmap

import numpy as np
import pytest

from tests import ogg_chain_cases as K
from tests import ogg_demux_batch as B
from tests.ogg_chain_cases import ECAP, EINVAL
from tests.ogg_pages import guarded_mapping


@pytest.mark.parametrize("name", ["1 link", "2 links", "3 links", "65 links", "three classes", "headers alone in the middle",
                                  "headers alone at the end", "unterminated packet, then a link", "255 segments",
                                  "zero segments", "70 KB comment in the middle"])
def test_links_of_a_valid_chain(name):
    """the walker's starts, the link count the corpus was built with, and every link demuxed as it is alone"""
    blob, n = K.chains()[name]
    ok = K.check_demux("host", [blob])
    assert len(ok) == n and all(ok), ok


def test_first_page_without_the_flag():
    """link 0 starts at the file's first byte whatever its first page says"""
    blob, n = K.chains()["first page without the flag"]
    ok = K.check_demux("host", [blob])
    assert len(ok) == n == 2 and ok[1]


def test_flag_on_a_later_page_of_the_same_serial():
    """the file is cut there; the second part starts at page number 2 and is VBM_EOGG"""
    blob, n = K.chains()["flag on a later page"]
    ok = K.check_demux("host", [blob])
    assert ok == [True, False] and n == 2                    # the first part is the three header packets


def test_multiplexed_start():
    """two beginning-of-stream pages in a row: a first link of one page (fewer than three packets) and a second that
    mixes two serial numbers"""
    blob, _ = K.chains()["multiplexed start"]
    links = K.links_of(blob)
    assert len(links) == 2 and len(K.split_pages(links[0])) == 1
    assert K.check_demux("host", [blob]) == [False, False]


@pytest.mark.parametrize("what", sorted(K.MIDDLE))
def test_corrupted_middle_link(what):
    assert sorted(K.MIDDLE) == sorted(K.middle_corruptions())
    assert K.check_demux("host", [K.middle_corruptions()[what]]) == K.MIDDLE[what]


def test_all_chains_as_one_batch():
    blobs = [b for b, _ in K.chains().values()] + list(K.middle_corruptions().values())
    ok = K.check_demux("host", blobs)
    assert len(ok) == sum(n for _, n in K.chains().values()) + sum(len(x) for x in K.MIDDLE.values())


def test_every_prefix_of_a_two_link_file_as_one_batch():
    """adjacent files: a read past a file's end meets the next prefix and shows as a wrong result.  A prefix that ends in
    link 1 gives link 0 intact and link 1 as vbm_ogg_demux judges those bytes"""
    l0, l1 = K.two_link_file()
    blob = l0 + l1
    blobs = [blob[:k] for k in range(len(blob) + 1)]
    fl, lo = K.run("host", blobs)
    want_fl, want_lo = K.expected(blobs)
    assert np.array_equal(fl, want_fl) and np.array_equal(lo, want_lo)
    p0 = len(K.split_pages(l1)[0])                                # link 1 starts once its first page is all there
    assert np.array_equal(np.diff(fl), [1 if k < len(l0) + p0 else 2 for k in range(len(blob) + 1)])
    # the links of the prefixes that reach into link 1, demuxed as one batch
    first = len(l0) + 1
    j0, data = int(fl[first]), np.frombuffer(b"".join(blobs), np.uint8)
    sub = lo[j0:]
    b = B.Batch("host", len(sub) - 1, int(sub[-1] - sub[0]))
    try:
        info, totals = b.scan(data, sub)
        res = b.fill(totals)
    finally:
        b.close()
    whole, seen, j = B.single(l0), set(), 0
    for k in range(first, len(blob) + 1):
        for link in K.links_of(blobs[k]):
            if link == l0:
                assert B.same(B.file_view(info, res, j), whole), k
            else:
                want = B.single(link)
                assert B.same(B.file_view(info, res, j), want), k
                seen.add("eogg" if want is None else len(want[3]))
            j += 1
    assert j == len(sub) - 1 and "eogg" in seen and len(seen) > 2     # VBM_EOGG and several shortened forms


def test_empty_and_short_files():
    for blobs in ([b""], [b"OggS" + b"\0" * 22], [b"", b"", K.small_links(3)[0], b""]):
        ok = K.check_demux("host", blobs)
        assert len(ok) == len(blobs) and ok == [len(b) > 26 for b in blobs]


def test_no_files():
    fl, lo = K.run("host", [], first=5)
    assert fl.tolist() == [0] and lo.tolist() == [5]


def test_more_files_than_one_scan_step():
    blobs = K.many_files()
    K.check_split("host", blobs)
    assert K.expected(blobs)[0][-1] == 1025 + 1 + 2 + 1


@pytest.mark.parametrize("first", range(8))
def test_file_starts_at_every_alignment(first):
    blobs = K.alignment_batch()
    K.check_demux("host", blobs, first)


def test_capacity_one_short_writes_nothing():
    blobs = [b for b, _ in K.chains().values()]
    data, offsets = B.pack(blobs)
    want_fl, want_lo = K.expected(blobs)
    total = int(want_fl[-1])
    c = K.Chain("host", len(blobs), len(data))
    try:
        r = c.split(data, offsets, total - 1)
        assert r.status == ECAP and not r.touched and r.canaries_ok
        assert np.array_equal(r.file_links, want_fl)
        r = c.split(data, offsets, total)
        assert r.status == 0 and r.touched and r.canaries_ok
        assert np.array_equal(r.file_links, want_fl) and np.array_equal(r.link_offsets, want_lo)
    finally:
        c.close()


def test_einval():
    lib = B._lib()
    h = C.c_void_p()
    for bad in ((0, 10), (-1, 10), (1, -1)):
        assert lib.vbm_host_ogg_chain_create(C.byref(h), *bad) == EINVAL
    assert lib.vbm_host_ogg_chain_create(None, 1, 10) == EINVAL
    data, offsets = B.pack(list(K.small_links(3)))
    c = K.Chain("host", 3, len(data))
    fl, lo = np.zeros(4, np.int64), np.zeros(9, np.int64)

    def call(n, off, null=None, cap=8):
        off = np.ascontiguousarray(off, np.int64)            # alive until the call returns
        ptrs = {"data": data.ctypes.data, "offsets": off.ctypes.data, "file_links": fl.ctypes.data, "link_offsets": lo.ctypes.data}
        if null:
            ptrs[null] = None
        return c.split_raw(n, ptrs["data"], ptrs["offsets"], ptrs["file_links"], ptrs["link_offsets"], cap)

    try:
        assert call(3, offsets) == 0
        assert call(4, list(offsets) + [offsets[-1]]) == EINVAL                         # above max_files
        assert call(-1, offsets) == EINVAL
        assert call(3, [-1] + list(offsets[1:])) == EINVAL
        assert call(3, [0, 9, 8, 10]) == EINVAL                                         # decreasing
        assert call(3, list(offsets[:3]) + [offsets[3] + 1]) == EINVAL                  # above max_bytes
        assert b"max_bytes" in lib.vbm_last_error()
        for null in ("offsets", "file_links", "link_offsets", "data"):                  # data: with bytes to read
            assert call(3, offsets, null=null) == EINVAL, null
        assert call(3, [7, 7, 7, 7], null="data") == 0                                  # ... and with none
        assert call(3, offsets, cap=-1) == EINVAL
        st = C.c_int()
        assert lib.vbm_ogg_chain_status(None, C.byref(st), None) == EINVAL
        assert lib.vbm_ogg_chain_status(c.h, None, None) == EINVAL
        # a host object in the device call
        assert lib.vbm_ogg_chain_split(c.h, 3, data.ctypes.data, offsets.ctypes.data, fl.ctypes.data, lo.ctypes.data, 8,
                                       None) == EINVAL
        assert b"vbm_ogg_chain_create" in lib.vbm_last_error()
    finally:
        c.close()
    lib.vbm_ogg_chain_destroy(None)


def test_split_never_reads_past_the_last_file():
    """the data ends where an unreadable page begins, and the last file ends in a page that promises more"""
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    a, b, c = K.small_links(3)
    pages = K.split_pages(c)
    cuts = [len(c) - 1, len(c) - len(pages[-1]) + 26, len(c) - len(pages[-1]) + 27, len(c) - len(pages[-1]) + 28, 0, 5]
    for cut in cuts:
        blobs = [a + b, c[:cut]] if cut else [a + b, b""]
        data, offsets = B.pack(blobs)
        m, base, cap = guarded_mapping(libc, len(data))
        ch = K.Chain("host", 2, len(data))
        try:
            at = base + cap - len(data)
            C.memmove(at, data.tobytes(), len(data))
            want_fl, want_lo = K.expected(blobs)
            r = ch.split(at, offsets, int(want_fl[-1]))
            assert r.status == 0 and np.array_equal(r.file_links, want_fl) and np.array_equal(r.link_offsets, want_lo), cut
        finally:
            ch.close()
            libc.mprotect(C.c_void_p(base + cap), C.c_size_t(mmap.PAGESIZE), 3)
            m.close()


def test_split_ogg_chain():
    import vorbis_aotuv_lancer_amd as v
    a, b, c = K.small_links(3)
    assert v.split_ogg_chain(a) == [a]
    assert v.split_ogg_chain(a + b + c) == [a, b, c]
    assert v.split_ogg_chain(b"") == [b""]
    for link in v.split_ogg_chain(K.chains()["three classes"][0]):
        assert v.demux_ogg(link)[0][0][:7] == b"\x01vorbis"


def test_demux_ogg_device_chained_on_the_host_twin():
    import vorbis_aotuv_lancer_amd as v
    a, b, c = K.small_links(3)
    bad = bytearray(b)
    bad[-1] ^= 1
    files = [a + b, c, b"", c + bytes(bad) + a]
    bt = v.demux_ogg_device(files, host=True, chained=True)
    assert bt.file_links.dtype == np.int64 and bt.file_links.tolist() == [0, 2, 3, 4, 7]
    assert [list(bt.links(f)) for f in range(4)] == [[0, 1], [2], [3], [4, 5, 6]]
    assert bt.names == ["file 0 link 0", "file 0 link 1", "file 1 link 0", "file 2 link 0", "file 3 link 0", "file 3 link 1",
                        "file 3 link 2"]
    assert bt.status == [0, 0, 0, K.EOGG, 0, K.EOGG, 0]
    for i, link in enumerate([a, b, c, None, c, None, a]):
        if link is not None:
            want = v.demux_ogg(link)
            offs, gp, eos = bt.runs(i)
            at = int(bt.payload_base[i])
            assert bt.headers[i] == want[0] and np.array_equal(offs - at, want[2]) and np.array_equal(gp, want[3])
            assert np.array_equal(bt.payload[at:at + int(bt.payload_bytes[i])], want[1]) and np.array_equal(eos, want[4])
    plain = v.demux_ogg_device([a, c], host=True)
    assert plain.file_links.tolist() == [0, 1, 2] and plain.names == ["file 0", "file 1"]
