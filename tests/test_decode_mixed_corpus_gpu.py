"""MixedDecoder on what the single-class Decoder is pinned on but tests/test_decode_mixed_gpu.py never gives it: every
family of the generated corpus (vm.CORPUS: residue 0, odd dimensions, 16 submaps, chained coupling, 64 modes, truncated
and random packets ...) as a class of one call, decoders whose caps a class fills exactly, and the README's loop for
live mounts (resync OggFeed -> class_for -> bind -> synthesis_runs) end to end.  The yardstick is the single-class
Decoder of each class fed the same packets in the same calls (tests/decode_mixed_cases.py: PerClass), for the live loop
also decode_ogg of every link; the status of the corpus packets is compared with the model's as well.  Every comparison
is exact.  tests/test_decode_mixed_corpus_cpu.py states from the model alone that the counts asserted here can be met."""
import numpy as np
import pytest
import torch

from tests import decode_mixed_cases as M
from tests import ogg_feed_resync_cases as R
from tests.decode_calls import runs_inputs
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu

RATES = [False, True]
RATE_IDS = ["full", "half"]
CORPUS_CAPS = dict(max_classes=20, max_channels=8, max_blocksize=4096)


@pytest.fixture(scope="module")
def whole_corpus():
    """the script of every corpus packet (the model decodes them all here, before any test's clock starts)"""
    return M.corpus_script(M.corpus_pick())


def corpus_counts(fams, sid, result):
    """per family: rows of the first call with status 0 and != 0, and the streams that returned samples in the second
    or third call, split into those with nonzero PCM and those without; the first call's status is the model's"""
    good, bad, heard, mute = ([0] * len(fams) for _ in range(4))
    for (k, i), s in sid.items():
        f = fams[k]
        (_, sm1, st1), (p2, _, st2), (p3, _, st3) = result[s]
        assert st1 == [f.status[i]], f"{f.name} packet {i}: status {st1}, model {f.status[i]}"
        assert sm1 == [0] and st2 == [0] and st3 == [f.status[i], 0], f"{f.name} packet {i}"
        good[k] += st1 == [0]
        bad[k] += st1 != [0]
        if p2.shape[1] + p3.shape[1] > 0:
            if p2.any() or p3.any():
                heard[k] += 1
            else:
                mute[k] += 1
    return good, bad, heard, mute


def test_every_corpus_family_as_a_class_of_one_call(cuda, whole_corpus):
    """1669 streams, one per corpus packet p, play [p, a, p, b] in three calls with no host wait in between: all p, all
    a, and the runs [p, b]; neighbouring rows are of different families, and the third call goes through the rows in
    reverse, so a workspace row changes class between calls"""
    import vorbis_aotuv_lancer_amd as v
    fams, script, sid, order = whole_corpus
    S = len(sid)
    assert S == 1669
    m = M.both(v, fams, script, S, 2 * S, cuda, compact=True, **CORPUS_CAPS)
    good, bad, heard, mute = corpus_counts(fams, sid, m.result)
    print(f"\ncorpus rows per family: good {min(good)}..{max(good)}, failing {min(bad)}..{max(bad)}, "
          f"streams with nonzero PCM {min(heard)}..{max(heard)}; {m.samples} samples compared")
    for k, f in enumerate(fams):
        assert good[k] >= 60 and bad[k] >= 4, (f.name, good[k], bad[k])
        if f.name == M.SILENT:
            assert heard[k] == 0 and mute[k] >= 30, (f.name, heard[k], mute[k])
        else:
            assert heard[k] >= 30, (f.name, heard[k])
    blocks = M.corpus_blocks(order)
    assert sorted(blocks) == [256, 512, 1024, 2048, 4096] and all(len(of) >= 2 for of in blocks.values())
    assert M.corpus_sandwiched(order)


def test_corpus_families_at_half_rate(cuda):
    """the same three calls at half rate on 14 streams per family: 12 whose packet has a nonzero model spectrum and 2
    whose packet fails (unpack is the full-rate one)"""
    import vorbis_aotuv_lancer_amd as v
    fams, script, sid, order = M.corpus_script(M.corpus_pick(loud=12, failing=2))
    S = len(sid)
    assert S == 14 * len(fams)
    m = M.both(v, fams, script, S, 2 * S, cuda, halfrate=True, compact=True, **CORPUS_CAPS)
    good, bad, heard, mute = corpus_counts(fams, sid, m.result)
    for k, f in enumerate(fams):
        assert (good[k], bad[k]) == (12, 2), f.name
        assert (heard[k] == 0 and mute[k] >= 12) if f.name == M.SILENT else heard[k] >= 12, (f.name, heard[k], mute[k])
    assert M.corpus_sandwiched(order)


@pytest.mark.parametrize("halfrate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("n", range(len(M.CAPS)), ids=["scratch", "channels", "bins"])
def test_caps_that_a_class_fills_exactly(cuda, n, halfrate):
    """scratch: the 3-channel 256 / 256 family with residue grouping 1 needs 384 bytes of partition classes, exactly
    max_channels * max_blocksize / 2, in rows between those of a mono class; channels: 8-channel rows of 256 bins under
    max_blocksize 512; bins: 2-channel rows of 2048 bins under max_channels 2.  Nine streams, five steps and a runs
    call"""
    import vorbis_aotuv_lancer_amd as v
    caps = M.CAPS[n][0]
    classes, script, of = M.caps_script(n)
    if n == 0:
        assert M.class_bytes(classes[0].setup) == caps["max_channels"] * caps["max_blocksize"] // 2 == 384
    m = M.both(v, classes, script, M.CAPS_ROWS, 5 * M.CAPS_ROWS, cuda, halfrate=halfrate, **caps)
    assert all(st == [0] * len(st) for r in m.result.values() for _, _, st in r)
    for s, r in m.result.items():
        assert len(r) == 6 and sum(p.shape[1] for p, _, _ in r) > 0
        assert any(p.any() for p, _, _ in r), f"stream {s} of class {of[s]} is silent"


# ---- the live loop ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mounts(cuda):
    """five mounts of links under 1.5 s of two classes (stereo 44100 q5, mono 8000 q5): three chains of three links that
    alternate between the classes, one stereo link alone, and a chain whose second link lacks an audio page of its
    middle -> (mount bytes, per mount its links as encoded, (mount, link) of the damaged one)"""
    import vorbis_aotuv_lancer_amd as v
    lengths = (60000, 52000, 44100, 48000, 24000, 56000)
    st = v.encode_ogg([synth_signal(2, 44100, n, seed=50 + i) for i, n in enumerate(lengths)], 44100, quality=0.5,
                      serialnos=list(range(101, 107)))
    mo = v.encode_ogg([synth_signal(1, 8000, n, seed=70 + i) for i, n in enumerate((11000, 9000, 7000, 10000))], 8000,
                      quality=0.5, serialnos=list(range(201, 205)))
    links = [[st[0], mo[0], st[1]], [mo[1], st[2], mo[2]], [st[3], mo[3], st[0]], [st[4]], [mo[0], st[5], mo[2]]]
    ap = R.audio_pages(st[5])
    assert len(ap) >= 3
    R.assert_no_stray_capture(st[5])
    lost = ap[len(ap) // 2]
    assert ap[0] < lost < ap[-1]
    blobs = [b"".join(x) for x in links]
    blobs[4] = mo[0] + R.without_pages(st[5], {lost}) + mo[2]
    for b, x in zip(blobs[:4], links[:4]):
        assert v.split_ogg_chain(b) == x
    return blobs, links, (4, 1)


def pushes(blobs, step=1000, slow=1, every=3):
    """the session's pushes [(ids, chunks, end flags)]: `step` bytes per mount, one byte for mount `slow` on every
    third push; a mount leaves when its bytes are through"""
    at, out, t = [0] * len(blobs), [], 0
    while any(a < len(b) for a, b in zip(at, blobs)):
        ids = [s for s, b in enumerate(blobs) if at[s] < len(b)]
        size = [1 if s == slow and t % every == every - 1 else step for s in ids]
        out.append((ids, [blobs[s][at[s]:at[s] + n] for s, n in zip(ids, size)],
                    [at[s] + n >= len(blobs[s]) for s, n in zip(ids, size)]))
        for s, n in zip(ids, size):
            at[s] += n
        t += 1
    return out


def test_live_loop_of_the_readme(cuda, mounts):
    """OggFeed(resync=True).push_all -> class_for and bind on a new link -> one MixedDecoder.synthesis_runs per result
    with gap=r.gap, with no host wait beyond the feed's own; then every result again through a Decoder per class"""
    import vorbis_aotuv_lancer_amd as v
    blobs, links, damaged = mounts
    n, cap = len(blobs), 2048
    plan = pushes(blobs)
    assert len(plan[-1][0]) == 1 and len(blobs[3]) < min(len(b) for b in blobs[:3])       # a mount ends early
    feed = v.OggFeed(n, max_call_bytes=n * 8192, max_page_carry=65307, resync=True)
    md = v.MixedDecoder(n, cap, max_classes=4, max_channels=2, max_blocksize=2048)
    link_of = np.full(n, -1)
    log, calls, mixes, headers = [], 0, 0, {}   # log: ("bind", slot, class, calls so far) | ("call", r, live, out, chans)
    for ids, chunks, end in plan:
        for r in feed.push_all(ids, chunks, end=end):
            assert not any(r.status)
            ready = (r.info["headers_ready"] != 0) & (r.link != link_of[r.ids])
            for i in np.flatnonzero(ready):                     # a new link: its class, added or found by its headers
                c = md.class_for(feed.headers(r.ids[i]))
                headers.setdefault(c, feed.headers(r.ids[i]))
                md.bind([r.ids[i]], [c])
                link_of[r.ids[i]] = r.link[i]
                log.append(("bind", int(r.ids[i]), c, calls))
            live = r.counts > 0
            if not live.any():
                continue
            P = int(r.counts[live].sum())
            assert P <= cap
            stride = max(int(k) * w for k, w in zip(r.counts[live], md.row_of(r.ids[live])))
            out = (torch.full((int(live.sum()), md.channels, stride), M.FILL_PLAYER, dtype=torch.float32, device=cuda),
                   *(torch.empty(k, dtype=torch.int32, device=cuda) for k in (int(live.sum()), P, P)))
            md.synthesis_runs(r.ids[live], r.counts[live], r.payload, r.offsets, granulepos=r.granulepos, eos=r.eos,
                              gap=r.gap, out=out)
            mixes += len(set(md.stream_class[r.ids[live]].tolist())) > 1
            log.append(("call", r, live, out, md.channels_of(r.ids[live])))
            calls += 1
    feed.close()
    assert len(md.classes) == len(headers) == 2 and mixes > 0   # some call's live set holds slots of both classes
    binds = [e for e in log if e[0] == "bind"]
    assert len(binds) == sum(len(x) for x in links)
    assert any(0 < e[3] < calls for e in binds)                 # a bind between two decode calls of a running session

    # everything is read here, after the last call
    got = [[] for _ in range(n)]                                # per slot and link: [(pcm, samples, status)] per call
    rows = []                                                   # per call: [(slot, [(packet, granulepos, eos, gap)])]
    marks, first = [], [False] * n                              # gap marks: (slot, link, the link's first packet?)
    for e in log:
        if e[0] == "bind":
            got[e[1]].append([])
            first[e[1]] = True
            continue
        _, r, live, (pcm, rs, sm, st), chans = e
        pcm, rs, sm, st = pcm.cpu().numpy(), rs.cpu().tolist(), sm.cpu().tolist(), st.cpu().tolist()
        data, offs = r.payload.cpu().numpy().tobytes(), r.offsets.cpu().tolist()
        gp, eo, gap = r.granulepos.cpu().tolist(), r.eos.cpu().tolist(), r.gap.cpu().tolist()
        at, call = 0, []
        for row, (slot, cnt) in enumerate(zip(r.ids[live].tolist(), r.counts[live].tolist())):
            ch = chans[row]
            assert np.all(pcm[row, ch:] == M.FILL_PLAYER) and np.all(pcm[row, :ch, rs[row]:] == M.FILL_PLAYER), slot
            got[slot][-1].append((pcm[row, :ch, :rs[row]], sm[at:at + cnt], st[at:at + cnt]))
            call.append((slot, [(data[offs[k]:offs[k + 1]], gp[k], eo[k], gap[k]) for k in range(at, at + cnt)]))
            for k in range(at, at + cnt):
                if gap[k]:
                    marks.append((slot, len(got[slot]) - 1, first[slot] and k == at))
            first[slot] = False
            at += cnt
        assert at == len(offs) - 1
        rows.append(call)
    md.close()

    # the gap marks: the feed marks the first packet of every later link of a chain (the bind restarts the stream there
    # anyway), and beside those exactly one packet, behind the lost page
    assert sorted(m[:2] for m in marks if m[2]) == [(s, k) for s in range(n) for k in range(1, len(links[s]))]
    assert [m[:2] for m in marks if not m[2]] == [damaged]

    # link by link against decode_ogg
    flat = [(s, k) for s in range(n) for k in range(len(links[s]))]
    want = v.decode_ogg([links[s][k] for s, k in flat])
    for (s, k), (ref, _) in zip(flat, want):
        assert len(got[s]) == len(links[s])
        assert all(stt == [0] * len(stt) for _, _, stt in got[s][k])
        pcm = np.concatenate([p for p, _, _ in got[s][k]], axis=1)
        ref = ref.cpu().numpy()
        if (s, k) == damaged:
            assert 0 < pcm.shape[1] < ref.shape[1]
        else:
            assert pcm.shape == ref.shape and np.array_equal(pcm.view(np.uint32), ref.view(np.uint32)), (s, k)

    # the same feed results through a Decoder per class, restarted where the mixed decoder binds
    ds = {c: v.DecodeSetup(h) for c, h in headers.items()}
    dec = {c: v.Decoder(ds[c], n, cap) for c in ds}
    cls, pending, it = {}, [], iter(rows)
    for e in log:
        if e[0] == "bind":
            cls[e[1]] = e[2]
            dec[e[2]].restart_streams([e[1]])
            continue
        call = next(it)
        for c in sorted({cls[s] for s, _ in call}):
            mine = [(s, run) for s, run in call if cls[s] == c]
            data, offs, gp, eo, gap = runs_inputs([r for _, r in mine], cuda)
            counts = [len(run) for _, run in mine]
            stride = max(counts) * dec[c].row
            out = (torch.full((len(mine), dec[c].channels, stride), M.FILL_PLAYER, dtype=torch.float32, device=cuda),
                   *(torch.empty(k, dtype=torch.int32, device=cuda) for k in (len(mine), sum(counts), sum(counts))))
            dec[c].synthesis_runs([s for s, _ in mine], counts, data, offs, granulepos=gp, eos=eo, gap=gap, out=out)
            pending.append((mine, counts, out))
    twin = [[] for _ in range(n)]                               # per slot: [(pcm, samples, status)] per call, all links
    for mine, counts, (pcm, rs, sm, st) in pending:
        pcm, rs, sm, st = pcm.cpu().numpy(), rs.cpu().tolist(), sm.cpu().tolist(), st.cpu().tolist()
        at = 0
        for row, ((s, _), cnt) in enumerate(zip(mine, counts)):
            assert np.all(pcm[row, :, rs[row]:] == M.FILL_PLAYER)
            twin[s].append((pcm[row, :, :rs[row]], sm[at:at + cnt], st[at:at + cnt]))
            at += cnt
    for d in dec.values():
        d.close()
    for d in ds.values():
        d.close()
    for s in range(n):
        mine = [x for link in got[s] for x in link]
        assert len(mine) == len(twin[s]) > 0
        for k, ((p, sm, st), (wp, wsm, wst)) in enumerate(zip(mine, twin[s])):
            assert sm == wsm and st == wst, f"slot {s}, call {k}: samples or status"
            assert p.shape == wp.shape and np.array_equal(p.view(np.uint32), wp.view(np.uint32)), f"slot {s}, call {k}"
