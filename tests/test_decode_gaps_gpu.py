"""Gap marks in the decoder (vbm_synthesis_runs_gaps, Decoder.synthesis_runs(gap=...)) on the MI355X: a mark makes the
stream lose count as vorbis_synthesis_blockin does when packets are out of sequence (lib/block.c:911-915), and nothing
else.  Sample counts are checked against the tests' one restatement of lib/block.c:907-915 and 1050-1161 (blockin in
tests/decode_packets.py), PCM bit for bit against today's path on the same packet list without marks, and the live
loop (resync OggFeed.push_all -> synthesis_runs) link by link."""
import numpy as np
import pytest

from tests import ogg_feed_resync_cases as R
from tests.decode_calls import runs_inputs
from tests.decode_packets import blockin
from tests.signals import burst_signal

pytestmark = pytest.mark.gpu


def blockin_counts(bs, W, gp_in, eos, gap):
    """tests/decode_packets.py's blockin for a list of valid packets from a fresh stream at full rate -> samples
    returned per packet.  W: block flag per packet; gp_in / eos: the packets' granule positions and end flags; gap: out
    of sequence here."""
    return blockin(bs, 0, [0] * len(W), W, gp_in, eos, gap)[0]


@pytest.fixture(scope="module")
def material(cuda):
    """three stereo 44.1 kHz q5 files with block switching: per file its packets [(bytes, granulepos, eos)], headers and
    block flags"""
    import vorbis_aotuv_lancer_amd as v
    files = v.encode_ogg([burst_signal(2, 44100, n, seed=60 + i, period=5000) for i, n in enumerate((60000, 50000, 40000))],
                         44100, quality=0.5, serialnos=[71, 72, 73])
    streams = []
    for f in files:
        pk, hdr = R.strict_packets(f)
        streams.append([p[:3] for p in pk])
    ds = v.DecodeSetup(hdr)
    dec = v.Decoder(ds, 3, 1024)
    out = decode(dec, [0, 1, 2], streams)
    assert not out[3].cpu().numpy().any()
    info = dec.fetch("info").cpu().numpy()
    flags, at = [], 0
    for s in streams:
        flags.append(info[at:at + len(s), 1].tolist())
        at += len(s)
    dec.close()
    assert all(0 in w and 1 in w for w in flags)
    return v, ds, files, streams, flags


def decode(dec, ids, runs, gaps=None, marks=True):
    """one synthesis_runs call.  gaps: per run the marks of its rows, which go to the call as a tensor even when all
    are zero; marks=False: the call is made without the gap argument"""
    if gaps is not None:
        runs = [[p + (g,) for p, g in zip(r, gs)] for r, gs in zip(runs, gaps)]
    data, offs, gp, eo, gap = runs_inputs(runs, "cuda", marks=gaps is not None)
    kw = {"gap": gap} if marks else {}
    return dec.synthesis_runs(ids, [len(r) for r in runs], data, offs, granulepos=gp, eos=eo, **kw)


def test_no_marks_is_todays_path(material):
    v, ds, _, streams, _ = material
    runs = [s[:12] for s in streams]                            # one class, three streams, 36 packets
    outs = []
    for gaps, marks in ((None, False), (None, True), ([[0] * 12] * 3, True)):
        dec = v.Decoder(ds, 3, 64)
        outs.append([t.cpu().numpy() for t in decode(dec, [0, 1, 2], runs, gaps, marks)])
        dec.close()
    for o in outs[1:]:
        assert np.array_equal(o[1], outs[0][1]) and np.array_equal(o[2], outs[0][2]) and np.array_equal(o[3], outs[0][3])
        for r in range(3):
            n = int(o[1][r])
            assert n > 0 and np.array_equal(o[0][r, :, :n].view(np.uint32), outs[0][0][r, :, :n].view(np.uint32))


def holes(W):
    """(first removed, first kept) for holes whose far side is: long after long, short after short, and a short / long
    transition in either direction"""
    want = {(1, 1): None, (0, 0): None, (1, 0): None, (0, 1): None}
    for k in range(4, len(W) - 3):                              # packets k - 2 and k - 1 go: k follows k - 3
        if want[(W[k - 3], W[k])] is None:
            want[(W[k - 3], W[k])] = (k - 2, k)
    assert all(want.values()), want
    return sorted(want.values())


def test_hole_counts_and_pcm(material):
    v, ds, _, streams, flags = material
    bs = ds.blocksizes
    for s, (pk, W) in enumerate(zip(streams, flags)):
        for a, b in holes(W):
            keep = list(range(a)) + list(range(b, len(pk)))
            spliced, Wk = [pk[k] for k in keep], [W[k] for k in keep]
            gap = [int(k == b) for k in keep]
            dec = v.Decoder(ds, 1, 1024)
            pcm, total, samples, status = (t.cpu().numpy() for t in decode(dec, [0], [spliced], [gap]))
            dec.close()
            dec = v.Decoder(ds, 1, 1024)
            pcm0, total0, samples0, status0 = (t.cpu().numpy() for t in decode(dec, [0], [spliced], None, False))
            dec.close()
            assert not status.any() and not status0.any()
            want = blockin_counts(bs, Wk, [p[1] for p in spliced], [p[2] for p in spliced], gap)
            assert samples.tolist() == want and int(total[0]) == sum(want), (s, a, b)
            assert samples[-1] == want[-1] and spliced[-1][2] == 1              # the end of the stream
            # the overlap-add does not depend on the bookkeeping: packet by packet the same bits as without marks, in
            # front of the last page-end granule position behind the hole
            marked = [k for k in range(a, len(spliced)) if spliced[k][1] != -1]
            assert marked, (s, a, b)
            at, at0 = np.concatenate([[0], np.cumsum(samples)]), np.concatenate([[0], np.cumsum(samples0)])
            for k in range(marked[-1]):
                assert samples[k] == samples0[k], (s, a, b, k)
                assert np.array_equal(pcm[0, :, at[k]:at[k + 1]].view(np.uint32), pcm0[0, :, at0[k]:at0[k + 1]].view(np.uint32))


def test_mark_on_an_error_row_goes_to_the_next_valid_packet(material):
    """the packet behind the hole does not parse: the stream still loses count at the next one that does, in the same
    call and in a later one"""
    v, ds, _, streams, flags = material
    pk, W = streams[0], flags[0]
    a, b = holes(W)[0]
    # the packet behind the error row is given the granule position -5: a stream that has lost count takes it as its
    # position and cuts 5 samples off the front (lib/block.c:1090-1118); one that counts on cuts by its own count
    good = pk[:a] + [(pk[b][0], -5, 0)] + pk[b + 1:]
    bad = good[:a] + [(b"\x01no audio", -1, 0)] + good[a:]
    want = blockin_counts(ds.blocksizes, W[:a] + W[b:], [p[1] for p in good], [p[2] for p in good],
                          [int(k == a) for k in range(len(good))])
    unmarked = blockin_counts(ds.blocksizes, W[:a] + W[b:], [p[1] for p in good], [p[2] for p in good], [0] * len(good))
    full = ds.blocksizes[W[a - 1]] // 4 + ds.blocksizes[W[b]] // 4
    assert want[a] == full - 5 != unmarked[a] and want[:a] == unmarked[:a]
    for split in (None, a + 1):                                   # one call; the error row ends the first of two calls
        dec = v.Decoder(ds, 1, 1024)
        gap = [int(k == a) for k in range(len(bad))]
        parts = [(bad, gap)] if split is None else [(bad[:split], gap[:split]), (bad[split:], gap[split:])]
        samples, status = [], []
        for rows, g in parts:
            out = decode(dec, [0], [rows], [g])
            samples += out[2].cpu().tolist()
            status += out[3].cpu().tolist()
        dec.close()
        assert status[a] != 0 and samples[a] == 0 and not any(status[:a] + status[a + 1:])
        assert samples[:a] + samples[a + 1:] == want, split


def test_live_loop_chained_mount_with_lost_pages(material):
    """two slots, each a chain of two links of the class with one page removed per link, 4096 bytes per slot and call"""
    v, ds, files, _, _ = material
    mounts, want = [], []
    for first, second in ((files[0], files[1]), (files[2], files[0])):
        links, left = [], []
        for f in (first, second):
            ap = R.audio_pages(f)
            assert len(ap) >= 3
            links.append(R.without_pages(f, {ap[len(ap) // 2]}))
            left.append(R.survivors(f, {ap[len(ap) // 2]}))
        mounts.append(b"".join(links))
        want.append(left)
    feed = v.OggFeed(2, 8192, resync=True)
    dec = v.Decoder(ds, 2, 1024)
    link_now, got = [-1, -1], [{}, {}]
    step = 4096
    for at in range(0, max(len(m) for m in mounts), step):
        ids = [s for s in range(2) if at < len(mounts[s])]
        for r in feed.push_all(ids, [mounts[s][at:at + step] for s in ids], end=[at + step >= len(mounts[s]) for s in ids]):
            assert not any(r.status)
            for i, slot in enumerate(r.ids.tolist()):
                if r.info[i]["headers_ready"] and int(r.link[i]) != link_now[slot]:      # a new link: its setup, a restart
                    new = v.DecodeSetup(feed.headers(slot))
                    assert (new.channels, new.rate, new.blocksizes) == (ds.channels, ds.rate, ds.blocksizes)
                    new.close()
                    dec.restart_streams([slot])
                    link_now[slot] = int(r.link[i])
            live = np.flatnonzero(r.counts)
            if not len(live):
                continue
            pcm, n, _, status = dec.synthesis_runs(r.ids[live], r.counts[live], r.payload, r.offsets, granulepos=r.granulepos,
                                                   eos=r.eos, gap=r.gap)
            assert not status.cpu().numpy().any()
            for row, (slot, k) in enumerate(zip(r.ids[live].tolist(), n.cpu().tolist())):
                got[slot].setdefault(link_now[slot], []).append(pcm[row, :, :k].cpu().numpy())
    feed.close()
    dec.close()
    for slot in range(2):
        assert sorted(got[slot]) == [0, 1]
        for k, left in enumerate(want[slot]):
            assert sum(p[3] for p in left) == 1                 # (a later link's first packet is marked too: a restart)
            ref = v.Decoder(ds, 1, 1024)
            pcm, n, _, status = decode(ref, [0], [[p[:3] for p in left]], [[p[3] for p in left]])
            ref.close()
            assert not status.cpu().numpy().any()
            assert np.array_equal(np.concatenate(got[slot][k], axis=1).view(np.uint32),
                                  pcm[0, :, :int(n[0])].cpu().numpy().view(np.uint32)), (slot, k)
