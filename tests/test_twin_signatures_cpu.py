"""The invariant _twin._TwinHandle._call rests on: the device form of an entry point takes what its host twin takes, or
that and one trailing void *stream.  The pairs that differ in more are listed, and the list is held to the table."""
import ctypes as C

from vorbis_aotuv_lancer_amd._lib import SIGNATURES

# the host twin takes the index as arrays and the device form a store's handle; the twin is made from a setup and its own
# rate and the device form from a decoder; only the device form takes classes
STRUCTURAL = {"ogg_cut_ranges", "live_store_create", "live_store_restart"}


def _pairs():
    stems = [name[len("vbm_host_"):] for name in SIGNATURES if name.startswith("vbm_host_")]
    return {s: (SIGNATURES["vbm_host_" + s], SIGNATURES["vbm_" + s]) for s in stems if "vbm_" + s in SIGNATURES}


def _obeys(host, device):
    return device[0] == host[0] and device[1] in (host[1], host[1] + [C.c_void_p])


def test_device_form_is_the_host_twin_plus_at_most_a_stream():
    pairs = _pairs()
    assert len(pairs) > len(STRUCTURAL) and STRUCTURAL <= set(pairs)
    breaks = {s for s, (host, device) in pairs.items() if not _obeys(host, device)}
    assert breaks == STRUCTURAL, (sorted(breaks - STRUCTURAL), sorted(STRUCTURAL - breaks))


def test_call_adds_the_stream_exactly_where_the_device_form_has_one_more_argument():
    from vorbis_aotuv_lancer_amd._twin import _entry
    for s, (host, device) in _pairs().items():
        assert _entry(s, True)[1:] == ("vbm_host_" + s, False)
        assert _entry(s, False)[1:] == ("vbm_" + s, len(device[1]) == len(host[1]) + 1)
