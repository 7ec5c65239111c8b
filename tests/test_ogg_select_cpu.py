"""The Vorbis stream of multiplexed Ogg files, on the host: the twin of vbm_ogg_select (vbm_host_ogg_select) against the
rule of csrc/ogg_select.h restated in Python (ogg_select_cases.model), select_vorbis_stream, and the multiplexed=True
paths of demux_ogg_device and decode_ogg as far as they need no GPU.  The device form: test_ogg_select_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import ogg_demux_batch as B
from tests import ogg_select_cases as S
from tests.ogg_select_cases import ECAP, EINVAL, EOGG


@pytest.mark.parametrize("group", S.GROUPS)
def test_host_twin_equals_the_model(group):
    """output bytes, offsets and every info field, into a buffer of exactly the kept total, guard behind it"""
    blobs = S.group(group)
    S.check_model("host", blobs)
    S.check_model("host", blobs, first=3, out_cap=sum(len(b) for b in blobs))      # the input's size always suffices


def test_alignment_corpus_covers_every_pair_and_length():
    """what the device copy's paths depend on: names what a change of the generator dropped"""
    pairs, lengths = S.alignment_coverage(S.alignment_files())
    assert not {(a, b) for a in range(16) for b in range(16)} - pairs
    assert not set(range(27, 27 + 65)) - lengths


def test_runs_fit_the_files_slots():
    """the workspace bound of ogg_select.h: a file of n bytes has at most n / 27 runs"""
    for group in S.GROUPS:
        for b in S.group(group):
            assert len(S.model(b)[2]) <= len(b) // 27


def test_select_vorbis_stream_equals_the_twin_on_single_files():
    import vorbis_aotuv_lancer_amd as v
    files = [m for _, m, _ in S.singles()] + list(S.case6().values()) + list(S.case8().values())
    for blob in files:
        assert v.select_vorbis_stream(blob) == S.run("host", [blob]).out.tobytes() == S.model(blob)[0]


@pytest.mark.parametrize("k", range(S.N_SINGLES))
def test_select_then_demux_equals_the_vorbis_only_file(k):
    """cases 1 to 5: the second yardstick.  The links of a chain one by one"""
    import vorbis_aotuv_lancer_amd as v
    name, blob, want = S.singles()[k]
    out = v.select_vorbis_stream(blob)
    got, ref = v.split_ogg_chain(out), v.split_ogg_chain(want)
    assert len(got) == len(ref) and (len(ref) > 1) == (name in S.case5())
    for g, r in zip(got, ref):
        one = B.single(r)
        assert one is not None and B.same(B.single(g), one)
    if len(ref) == 1:
        h, data, offs, gp, eos = v.demux_ogg(out)
        h2, data2, offs2, gp2, eos2 = v.demux_ogg(want)
        assert h == h2 and np.array_equal(data, data2) and np.array_equal(offs, offs2)
        assert np.array_equal(gp, gp2) and np.array_equal(eos, eos2)


def test_first_vorbis_stream_of_a_group_wins():
    for name, (blob, want) in S.case4().items():
        out, info, _ = S.model(blob)
        r = S.run("host", [blob])
        assert r.out.tobytes() == want == out, name
        assert r.info["streams"][0] == 1 and r.info["foreign_streams"][0] >= 1     # the second Vorbis head page is foreign


def test_reused_serial_numbers_are_still_foreign():
    """case 5: group 2 has a foreign stream under the serial number group 1 chose, and one under group 1's foreign one"""
    blob, want = S.case5()["three groups"]
    r = S.run("host", [blob])
    assert r.out.tobytes() == want and r.info["streams"][0] == 3


def test_a_group_without_vorbis_keeps_nothing():
    blob, want = S.case5()["a group without vorbis in the middle"]
    r = S.run("host", [blob])
    assert r.out.tobytes() == want and r.info["streams"][0] == 2
    r = S.run("host", list(S.case6().values()))
    assert len(r.out) == 0 and not r.out_offsets.any()
    assert not r.info["streams"].any() and not r.info["kept_pages"].any() and r.info["foreign_pages"].all()


def test_plain_files_and_chains_come_out_as_they_went_in():
    """case 7: the same bytes at the same offsets"""
    blobs = list(S.case7().values())
    data, offsets = B.pack(blobs)
    r = S.run("host", blobs)
    assert r.out.tobytes() == data.tobytes() and np.array_equal(r.out_offsets, offsets)
    assert not r.info["foreign_pages"].any() and not r.info["foreign_streams"].any()


def test_no_vorbis_stream_is_an_empty_entry_with_its_message():
    """case 6 through the host paths: the demux rejects the empty entry, and the error says why"""
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd import decoder
    good = S.case1()["skeleton first"][0]
    files = [good] + list(S.case6().values())
    b = v.demux_ogg_device(files, host=True, multiplexed=True)
    assert b.status == [0] + [EOGG] * len(S.case6())
    assert b.select_info["streams"].tolist() == [1] + [0] * len(S.case6())
    with pytest.raises(v.VbmError, match="file 1: no Vorbis stream"):
        decoder._raise_failed(b, b.names)
    b = v.demux_ogg_device(files, host=True, multiplexed=True, chained=True)
    assert b.status == [0] + [EOGG] * len(S.case6()) and b.file_links.tolist() == list(range(len(files) + 1))
    with pytest.raises(v.VbmError, match="file 1 link 0: no Vorbis stream"):
        decoder._raise_failed(b, b.names)
    for chained in (False, True):
        with pytest.raises(v.VbmError, match="file 1: no Vorbis stream"):
            decoder._demux_files(files, False, chained, True)
    with pytest.raises(v.VbmError):
        v.demux_ogg(v.select_vorbis_stream(files[1]))       # the demux's own rejection of the empty file


def test_argument_checks():
    lib = B._lib()
    blob = S.case1()["skeleton first"][0]
    data, off = B.pack([blob])
    s = S.Select("host", 2, len(blob))
    other = S.Select("host", 1, 10)
    try:
        out, oo = np.zeros(len(blob) + 16, np.uint8), np.zeros(4, np.int64)
        info = np.zeros(2, S.info_dtype())
        ok = (1, data.ctypes.data, off.ctypes.data, out.ctypes.data, len(blob), oo.ctypes.data, info.ctypes.data)
        assert s.select_raw(*ok) == 0

        def bad(**kw):
            names = ("nfiles", "data", "off", "out", "out_cap", "out_off", "info")
            args = [kw.get(n, a) for n, a in zip(names, ok)]
            return s.select_raw(*args)

        assert bad(nfiles=-1) == EINVAL and bad(nfiles=3) == EINVAL
        assert bad(data=None) == EINVAL and bad(off=None) == EINVAL and bad(out=None) == EINVAL
        assert bad(out_off=None) == EINVAL and bad(info=None) == EINVAL and bad(out_cap=-1) == EINVAL
        assert b"null" in lib.vbm_last_error() or b"negative" in lib.vbm_last_error()
        for wrong in ([-1, 5], [9, 5]):
            o = np.array(wrong, np.int64)
            assert bad(off=o.ctypes.data) == EINVAL
        assert other.select_raw(*ok) == EINVAL and b"max_bytes" in lib.vbm_last_error()      # the span is above max_bytes
        # not in place: an output that overlaps the files
        assert bad(out=data.ctypes.data + len(blob) - 1) == EINVAL and b"overlaps" in lib.vbm_last_error()
        assert bad(out=data.ctypes.data, out_cap=1) == EINVAL
        # a device call needs the device form
        assert lib.vbm_ogg_select(s.h, *ok, None) == EINVAL and b"vbm_ogg_select_create" in lib.vbm_last_error()
        # what may be null: the data of an empty span, the output of capacity 0, the info of no file
        z = np.zeros(2, np.int64)
        assert s.select_raw(1, None, z.ctypes.data, None, 0, oo.ctypes.data, info.ctypes.data) == 0
        assert s.select_raw(0, None, z.ctypes.data, None, 0, oo.ctypes.data, None) == 0 and s.status() == 0
        st = C.c_int()
        assert lib.vbm_ogg_select_status(None, C.byref(st), None) == EINVAL
        assert lib.vbm_ogg_select_status(s.h, None, None) == EINVAL
        h = C.c_void_p()
        assert lib.vbm_host_ogg_select_create(C.byref(h), 0, 10) == EINVAL
        assert lib.vbm_host_ogg_select_create(C.byref(h), 1, -1) == EINVAL
        assert lib.vbm_host_ogg_select_create(None, 1, 1) == EINVAL
    finally:
        s.close()
        other.close()


def test_a_short_output_buffer_is_ecap_and_nothing_is_written():
    blobs = [m for _, m, _ in S.singles()][:3]
    data, offsets = B.pack(blobs)
    want_out, want_off, want_info = S.expected(blobs)
    s = S.Select("host", len(blobs), len(data))
    try:
        r = s.select(data, offsets, len(want_out) - 1)
        assert r.status == ECAP and not r.touched and r.guard_ok
        assert np.array_equal(r.out_offsets, want_off) and S.same_info(r.info, want_info)     # these are always written
        r = s.select(data, offsets, len(want_out))
        assert r.status == 0 and r.out.tobytes() == want_out and r.guard_ok
    finally:
        s.close()


def _same_batch(got, want):
    assert got.status == want.status and got.headers == want.headers
    assert np.array_equal(got.file_links, want.file_links)
    for name in ("payload", "offsets", "granulepos", "eos"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert got.info.tobytes() == want.info.tobytes()


def test_demux_ogg_device_host_multiplexed():
    import vorbis_aotuv_lancer_amd as v
    one = [s for s in S.singles() if s[0] not in S.case5()]
    got = v.demux_ogg_device([m for _, m, _ in one], host=True, multiplexed=True)
    want = v.demux_ogg_device([w for _, _, w in one], host=True)
    assert not any(got.status) and want.select_info is None
    _same_batch(got, want)
    assert got.select_info["kept_bytes"].tolist() == [len(w) for _, _, w in one]
    # chains
    c5 = list(S.case5().values())
    got = v.demux_ogg_device([m for m, _ in c5], host=True, chained=True, multiplexed=True)
    want = v.demux_ogg_device([w for _, w in c5], host=True, chained=True)
    assert not any(got.status) and got.file_links.tolist() == [0, 2, 5, 7]
    _same_batch(got, want)
    assert got.names == want.names


def test_decode_ogg_host_demux_path_multiplexed():
    """decode_ogg's demux on the host (device_demux=False) up to where the GPU starts"""
    from vorbis_aotuv_lancer_amd import decoder
    for chained, cases in ((False, [s[1:] for s in S.singles() if s[0] not in S.case5()]), (True, list(S.case5().values()))):
        names, got, links = decoder._demux_files([m for m, _ in cases], False, chained, True)
        names2, want, links2 = decoder._demux_files([w for _, w in cases], False, chained)
        assert names == names2 and list(links) == list(links2) and len(got) == len(want)
        for g, w in zip(got, want):
            assert g[0] == w[0] and all(np.array_equal(a, b) for a, b in zip(g[1:], w[1:]))


def test_defaults_are_unchanged():
    """without the keyword a multiplexed file is refused as before, and as csrc/ogg_chain.h pins it with chained=True"""
    import vorbis_aotuv_lancer_amd as v
    files = [m for _, m, _ in S.singles()]
    b = v.demux_ogg_device(files, host=True)
    assert b.status == [EOGG] * len(files) and b.select_info is None
    blob = S.case1()["skeleton first"][0]
    b = v.demux_ogg_device([blob], host=True, chained=True)
    assert b.status == [EOGG, EOGG] and b.file_links.tolist() == [0, 2]
    with pytest.raises(v.VbmError):
        v.demux_ogg(blob)
    with pytest.raises(ValueError, match="multiplexed"):
        v.read_ogg(blob)
