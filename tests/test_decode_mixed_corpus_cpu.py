"""What tests/test_decode_mixed_corpus_gpu.py asserts about its own inputs, stated from the model alone (no GPU): the
generated corpus (vm.CORPUS) gives every family enough rows that decode, that fail and that carry a nonzero spectrum, the
first call's block lists mix families at every transform size, a failing row lies between good rows of other families,
and the classes of the cap tests fill the caps they are meant to fill."""
import pytest

from tests import decode_mixed_cases as M
from tests import vorbis_model as vm

K = range(len(vm.CORPUS))
NAMES = [n for n, _ in vm.CORPUS]


def test_every_family_has_good_failing_and_loud_rows():
    total = 0
    for k in K:
        f = M.family(k)
        good, bad, loud = f.status.count(0), len(f.status) - f.status.count(0), sum(f.loud)
        total += len(f.packets)
        assert 68 <= len(f.packets) <= 91, (f.name, len(f.packets))
        assert good >= 60 and bad >= 4, (f.name, good, bad)
        if f.name == M.SILENT:
            assert loud == 0
        else:
            assert loud >= 30, (f.name, loud)
    assert total == 1669 and M.SILENT in NAMES


@pytest.mark.parametrize("k", K, ids=NAMES)
def test_the_whole_packets_decode_and_have_every_block_flag(k):
    f = M.family(k)
    flags = sorted({md[0] for md in f.setup["modes"]})
    for seed in range(5):                                       # seed 0: the corpus script; 0 .. 4: the cap tests' streams
        a, b = M.whole(k, seed)
        ra, rb = f.model.decode(a), f.model.decode(b)
        assert ra["status"] == 0 and rb["status"] == 0
        assert [f.W(a), f.W(b)] == [flags[0], flags[-1]] and (a is b) == (len(flags) == 1)
        assert bool(ra["spectrum"].any()) == bool(rb["spectrum"].any()) == (f.name != M.SILENT)
    assert len(M.family_stream(k, 1)) == len(M.SEQ)


def test_first_call_mixes_families_on_every_block_list_and_around_a_failing_row():
    fams, script, sid, order = M.corpus_script(M.corpus_pick())
    assert len(order) == len(sid) == 1669 and sorted(sid.values()) == list(range(1669))
    assert [k for k, _ in order[:len(fams)]] == list(K)         # round-robin: neighbours are of different families
    assert [s for s, _ in script[-1][1]] == [s for s, _ in script[-2][1]][::-1]
    blocks = M.corpus_blocks(order)
    assert sorted(blocks) == [256, 512, 1024, 2048, 4096]
    for size, of in blocks.items():
        assert len(of) >= 2, (size, of)
    assert M.corpus_sandwiched(order)


def test_half_rate_subset_keeps_every_family():
    pick = M.corpus_pick(loud=12, failing=2)
    for k in K:
        f = M.family(k)
        assert len(pick[k]) == 14 and sum(f.status[i] != 0 for i in pick[k]) == 2
        assert sum(f.loud[i] for i in pick[k]) == (0 if f.name == M.SILENT else 12)
    order = M.corpus_script(pick)[3]
    assert all(len(of) >= 2 for of in M.corpus_blocks(order).values()) and M.corpus_sandwiched(order)


def test_the_cap_classes_fill_their_caps():
    first = M.family(0)
    assert (first.ch, first.bs) == (3, (256, 256)) and first.setup["residues"][0]["grouping"] == 1
    assert M.class_bytes(first.setup) == 384 == 3 * 256 // 2    # exactly max_channels * max_blocksize / 2
    assert M.CAPS[0][0] == dict(max_channels=3, max_blocksize=256)
    for n, (caps, names, _) in enumerate(M.CAPS):
        classes, script, of = M.caps_script(n)
        assert max(c.ch for c in classes) == caps["max_channels"]
        assert max(c.bs[1] for c in classes) == caps["max_blocksize"]
        assert all(M.class_bytes(M.family_named(x).setup) <= caps["max_channels"] * caps["max_blocksize"] // 2
                   for x in names)
        assert len(of) == 9 and set(of) == set(range(len(classes)))
        assert all(len(rows) == 9 for kind, rows in script[-6:])
    _, _, of = M.caps_script(0)                                 # the family that fills its scratch has neighbours
    assert of == [1, 0, 1, 0, 1, 0, 1, 0, 1]
