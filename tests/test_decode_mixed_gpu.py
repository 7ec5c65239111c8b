"""MixedDecoder (vbm_decoder_create_mixed): streams of different header classes in one call.  The yardstick everywhere
is the single-class Decoder fed the same packets of the same stream in the same calls (tests/decode_mixed_cases.py:
PerClass), which the other decode suites pin bit for bit; PCM (the used channels and samples), samples, run_samples
and status are compared exactly, and a stream writes nothing outside its own channels and samples."""
import numpy as np
import pytest
import torch

from tests import decode_mixed_cases as M
from tests.decode_calls import rows_tensor
from tests.decode_packets import ogg_packets
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu

RATES = [False, True]
RATE_IDS = ["full", "half"]


def step_script(streams):
    """streams {stream id: [packets]} -> batch events, one packet per stream per call while it lasts"""
    T = max(len(pk) for pk in streams.values())
    return [("batch", [(s, pk[t]) for s, pk in streams.items() if t < len(pk)]) for t in range(T)]


@pytest.fixture(scope="module")
def encoded(cuda):
    """five real files of two header classes (stereo 44100 q5, mono 8 kHz), each under 2 s, and decode_ogg's PCM"""
    import vorbis_aotuv_lancer_amd as v
    stereo = v.encode_ogg([synth_signal(2, 44100, n, seed=3 + i) for i, n in enumerate((40001, 30000, 4099))], 44100,
                          quality=0.5, serialnos=[11, 12, 13])
    mono = v.encode_ogg([synth_signal(1, 8000, n, seed=8 + i) for i, n in enumerate((15000, 2500))], 8000, quality=0.5,
                        serialnos=[21, 22])
    files = [stereo[0], mono[0], stereo[1], stereo[2], mono[1]]
    return files, v.decode_ogg(files)


def test_one_class_equals_the_decoder(cuda, encoded):
    """a synthetic class packet by packet and in runs, and a real one in runs; the last packets carry granule positions
    and e_o_s, so the end trim runs"""
    import vorbis_aotuv_lancer_amd as v
    k = M.synthetic(2, (256, 2048))
    streams = {0: M.stream(2, (256, 2048)), 1: M.stream(2, (256, 2048), contrary=True), 2: M.stream(2, (256, 2048), seed=5)}
    start = [("add", 0), ("bind", [0, 1, 2], [0, 0, 0])]
    M.both(v, [k], start + step_script(streams), 3, 8, cuda)
    runs = [("runs", [(s, list(pk[:4])) for s, pk in streams.items()]),
            ("runs", [(s, list(pk[4:])) for s, pk in streams.items()])]
    m = M.both(v, [k], start + runs, 3, 32, cuda)
    assert [sum(len(sm) for _, sm, _ in m.result[s]) for s in range(3)] == [10, 10, 10]
    assert m.result[0][-1][1][-1] < 1024 + 128                 # the trimmed last packet
    headers, pk = ogg_packets(encoded[0][3])                 # 4099 stereo samples
    assert 3 <= len(pk) <= 40 and pk[-1][2] == 1 and pk[-1][1] == 4099
    real = M.Class(headers, 2, (256, 2048))
    m = M.both(v, [real], [("add", 0), ("bind", [0], [0]), ("runs", [(0, pk)])], 1, 64, cuda, max_channels=2,
               max_blocksize=2048)
    assert m.samples == 4099


@pytest.mark.parametrize("halfrate", RATES, ids=RATE_IDS)
def test_channel_mix_at_equal_sizes(cuda, halfrate):
    """mono, stereo and 6 channels at 256 / 2048, a stream each, interleaved in every call: a step of short blocks puts
    1 + 2 + 6 = 9 blocks on the 256 list and the closing runs call 18, more than the 8 (at half rate 16) of one
    wavefront's group and no multiple of them, so one group holds blocks of rows of three classes and the last group
    is partial"""
    import vorbis_aotuv_lancer_amd as v
    bs = (256, 2048)
    classes = [M.synthetic(ch, bs) for ch in (1, 2, 6)]
    streams = {s: M.stream(k.ch, bs, seed=s) for s, k in enumerate(classes)}
    script = [("add", 0), ("add", 1), ("add", 2), ("bind", [2, 0, 1], [2, 0, 1])]
    script += step_script(streams)[:5] + [("runs", [(s, list(pk[5:])) for s, pk in streams.items()])]
    m = M.both(v, classes, script, 3, 16, cuda, halfrate=halfrate, count=True)
    group = 512 // ((256 >> halfrate) // 4)                      # blocks of 256 in a 512-complex group: 8, or 16
    small = [sum(ch for _, _, ch in call.get(256, [])) for call in m.blocks]
    assert any(n > group and n % group for n in small), small
    assert all(st == [0] * len(st) for r in m.result.values() for _, _, st in r)
    assert any({c for c, _, _ in call.get(256, [])} == {0, 1, 2} for call in m.blocks)


COLLIDING = [(2, (256, 512)), (1, (512, 512)), (3, (512, 4096)), (2, (4096, 4096)), (1, (1024, 2048))]


@pytest.mark.parametrize("halfrate", RATES, ids=RATE_IDS)
def test_size_collisions(cuda, halfrate):
    """block sizes that are long in one class and short in another, in one call: the 512 list takes the long rows of
    (256, 512) and the short rows of (512, 512) and (512, 4096); the 4096 kernel and the templated one run in the same
    call"""
    import vorbis_aotuv_lancer_amd as v
    classes = [M.synthetic(ch, bs) for ch, bs in COLLIDING]
    streams = {s: M.stream(k.ch, k.bs, seed=s) for s, k in enumerate(classes)}
    ids = list(streams)
    script = [("add", c) for c in ids] + [("bind", ids, ids)]
    script += [("runs", [(s, list(pk[:6])) for s, pk in streams.items()])] + step_script({s: pk[6:] for s, pk in streams.items()})
    m = M.both(v, classes, script, len(ids), 40, cuda, halfrate=halfrate, count=True)
    assert all(st == [0] * len(st) for r in m.result.values() for _, _, st in r)
    first = m.blocks[0]                                          # the runs call: six packets of every stream
    in512 = {(c, W) for c, W, _ in first[512]}
    assert (0, 1) in in512 and (2, 0) in in512 and any(c == 1 for c, _ in in512), in512
    assert 4096 in first and {256, 512, 1024, 2048} & set(first)
    assert {c for c, _, _ in first[4096]} == {2, 3}


@pytest.mark.parametrize("halfrate", RATES, ids=RATE_IDS)
def test_runs_of_1_2_7_and_30(cuda, halfrate):
    """per-run counts 1, 2, 7 and 30 in one call that starts every stream; inside the runs a truncated packet, a header
    packet (status != 0) and a gap mark; a second and a third call carry the padded tails on"""
    import vorbis_aotuv_lancer_amd as v
    spec = [(1, (256, 2048), 8), (6, (512, 1024), 8), (2, (256, 2048), 12), (3, (1024, 4096), 40)]
    classes, of = [], []
    for ch, bs, _ in spec:
        k = M.synthetic(ch, bs)
        if k not in classes:
            classes.append(k)
        of.append(classes.index(k))
    streams = [list(M.stream(ch, bs, seq=M.sequence(n), seed=20 + s)) for s, (ch, bs, n) in enumerate(spec)]
    whole = streams[3][4][0]
    streams[3][4] = (whole[:len(whole) // 2], -1, 0)             # truncated
    streams[3][9] = (classes[of[3]].headers[2], -1, 0)           # not an audio packet
    streams[2][3] = (b"", -1, 0)
    streams[3][17] = streams[3][17] + (1,)                       # packets were lost in front of this one
    streams[2][8] = streams[2][8] + (1,)
    cuts = [(0, 1, 4, 8), (0, 2, 5, 8), (0, 7, 10, 12), (0, 30, 35, 40)]
    script = [("add", c) for c in range(len(classes))] + [("bind", [0, 1, 2, 3], of)]
    for call in range(3):
        script.append(("runs", [(s, streams[s][cuts[s][call]:cuts[s][call + 1]]) for s in (3, 0, 2, 1)]))
    m = M.both(v, classes, script, 4, 40, cuda, halfrate=halfrate)
    status = [st for _, _, st in m.result[3]]
    assert status[0][9] != 0 and any(status[0][:4]) is False
    assert m.result[2][0][2][3] != 0
    assert [len(m.result[s][0][1]) for s in range(4)] == [1, 2, 7, 30]
    assert all(m.result[s][k][0].shape[1] > 0 for s in range(4) for k in (1, 2))


def test_rebind_to_a_smaller_class_after_calls_have_run(cuda):
    """a stream fills its tail at the caps (five long blocks of 8 channels x 4096), is then bound to a mono 256 / 1024
    class that joins the table only then, with no host wait in between, and decodes as on a fresh Decoder"""
    import vorbis_aotuv_lancer_amd as v
    classes = [M.synthetic(8, (1024, 4096)), M.synthetic(1, (256, 1024))]
    big = M.stream(8, (1024, 4096), seq="LLLLLL", seed=31)
    small = M.stream(1, (256, 1024), seed=32)
    other = M.stream(8, (1024, 4096), seed=33)
    assert [classes[0].W(p[0]) for p in big] == [1] * 6
    script = [("add", 0), ("bind", [0, 1], [0, 0]),
              ("runs", [(0, list(big[:3])), (1, list(other[:5]))]), ("runs", [(0, list(big[3:])), (1, list(other[5:7]))]),
              ("add", 1), ("bind", [0], [1]),
              ("runs", [(0, list(small[:4])), (1, list(other[7:]))])] + step_script({0: small[4:]})
    m = M.both(v, classes, script, 2, 16, cuda)
    assert sum(p.shape[1] for p, _, _ in m.result[0][:2]) == 5 * 2048 - 37          # the last packet is trimmed
    assert m.result[0][2][1][0] == 0 and m.result[0][2][0].shape[0] == 1     # the first packet after the bind


def test_six_calls_in_flight(cuda):
    """six calls back to back with no host wait, more than the four staging slots; 65 rows, and exactly max_batch"""
    import vorbis_aotuv_lancer_amd as v
    kinds = [(1, (256, 1024)), (2, (256, 2048)), (6, (256, 2048))]
    classes = [M.synthetic(ch, bs) for ch, bs in kinds]
    S, cap = 65, 96
    of = [s % 3 for s in range(S)]
    pk = {s: M.stream(*kinds[of[s]], seed=40 + s % 2) for s in range(S)}
    ids = list(range(S))
    script = [("add", 0), ("add", 1), ("add", 2), ("bind", ids[:40], of[:40]), ("bind", ids[40:], of[40:])]
    script.append(("batch", [(s, pk[s][0]) for s in ids]))                               # 65 rows
    script.append(("runs", [(s, list(pk[s][1:3 if s < cap - S else 2])) for s in ids]))  # 31 x 2 + 34 x 1 = 96 rows
    at = {s: 3 if s < cap - S else 2 for s in ids}
    for step in range(4):
        script.append(("batch" if step % 2 else "runs",
                       [(s, pk[s][at[s] + step] if step % 2 else [pk[s][at[s] + step]]) for s in ids[::-1]]))
    assert sum(len(r) for _, r in script[6][1]) == cap
    m = M.both(v, classes, script, S, cap, cuda)
    assert len(m.result) == S and all(len(r) == 6 for r in m.result.values())


def test_arguments(cuda, encoded):
    import vorbis_aotuv_lancer_amd as v
    small, wide, big = M.synthetic(2, (256, 512)), M.synthetic(6, (256, 2048)), M.synthetic(1, (1024, 2048))
    other = M.synthetic(1, (256, 512))
    ds = {k: v.DecodeSetup(k.headers) for k in (small, wide, big, other)}
    md = v.MixedDecoder(4, 8, max_classes=3, max_channels=2, max_blocksize=1024)
    with pytest.raises(v.VbmError, match="max_channels"):
        md.add_class(ds[wide])
    with pytest.raises(v.VbmError, match="max_blocksize"):
        md.add_class(ds[big])
    assert md.add_class(ds[small]) == 0 and md.add_class(ds[other]) == 1
    assert md.class_for(small.headers) == 2 and md.class_for(small.headers) == 2     # added once, then found
    with pytest.raises(v.VbmError, match="full"):
        md.add_class(ds[small])
    with pytest.raises(v.VbmError, match="class id"):
        md.bind([0], [3])
    md.bind([0, 1], [0, 1])
    assert md.channels_of([1, 0]) == [1, 2] and md.rate_of([0]) == [ds[small].rate]
    pk = M.stream(2, (256, 512))
    rows, nb = rows_tensor([pk[0][0], pk[1][0]], cuda)
    pcm = torch.full((2, 2, 512), M.FILL_PLAYER, dtype=torch.float32, device=cuda)
    ints = torch.full((4,), -5, dtype=torch.int32, device=cuda)
    with pytest.raises(v.VbmError, match="not bound"):         # stream 2 was never bound: nothing is enqueued
        md.synthesis_batch([0, 2], rows, nb, out=(pcm, ints[:2], ints[2:]))
    data = torch.zeros(16, dtype=torch.uint8, device=cuda)
    with pytest.raises(v.VbmError, match="not bound"):
        md.synthesis_runs([3], [1], data, torch.tensor([0, 16], device=cuda))
    torch.cuda.synchronize()
    assert (pcm == M.FILL_PLAYER).all() and (ints == -5).all()
    _, samples, status = md.synthesis_batch([0], rows[:1], nb[:1])        # the decoder still works
    assert status.cpu().tolist() == [0] and samples.cpu().tolist() == [0]
    with pytest.raises(v.VbmError, match="mixed"):
        md.fetch("spectrum")
    stream = (np.zeros(4, np.uint8), np.array([0, 4], np.int64), None, None)
    with pytest.raises(v.VbmError, match="mixed"):
        v.RangeStore(md, [stream])
    one = v.Decoder(ds[small], 1, 8)
    store = v.RangeStore(one, [stream])
    with pytest.raises(v.VbmError, match="mixed"):
        md.synthesis_ranges(store, [0], [0], [16])
    with pytest.raises(v.VbmError, match="mixed"):
        v.decode_index_device(md, data, torch.tensor([0, 16], device=cuda))
    for bad in (dict(max_channels=9), dict(max_blocksize=128), dict(max_blocksize=3000), dict(max_classes=0)):
        with pytest.raises(v.VbmError):
            v.MixedDecoder(1, 1, **bad)
    store.close()
    one.close()
    md.close()
    for d in ds.values():
        d.close()
    with pytest.raises(ValueError, match="one header class"):   # an index still takes one class
        v.OggIndex(encoded[0][:2])


def same_files(got, want):
    assert len(got) == len(want)
    for i, ((a, ra), (b, rb)) in enumerate(zip(got, want)):
        assert ra == rb and a.shape == b.shape and torch.equal(a, b), i


@pytest.mark.parametrize("halfrate", RATES, ids=RATE_IDS)
def test_decode_ogg_through_one_decoder(cuda, encoded, halfrate):
    import vorbis_aotuv_lancer_amd as v
    files, want = encoded
    if halfrate:
        want = v.decode_ogg(files, halfrate=True)
    for mp in (4096, 37):
        same_files(v.decode_ogg(files, max_packets=mp, halfrate=halfrate, one_decoder=True), want)
    if not halfrate:
        same_files(v.decode_ogg(files, device_demux=True, one_decoder=True), want)
        chain = files[3] + files[4] + files[2]                  # links of stereo, mono, stereo
        links = v.decode_ogg([chain, files[1]], chained=True, one_decoder=True)
        assert [len(x) for x in links] == [3, 1]
        same_files(links[0] + links[1], [want[3], want[4], want[2], want[1]])
        same_files(sum(v.decode_ogg([chain, files[1]], chained=True), []), links[0] + links[1])
