"""The directed corpora through the large-batch kernel variants (tests/large_batch.py): per-block path only, batches
just above the launchers' limits, everything large stays on the device.  Each test holds every replica to its signal's
first copy on the device and the first copies to the oracle, stage by stage, `post` included, and asserts from the
masks the runner collected that every block type of the class really ran in every large form it has."""
import pytest

from tests import large_batch as lb
from tests.large_batch import CASE_IDS, CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_large_batch(oracle, cuda, monkeypatch, c):
    from vorbis_aotuv_lancer_amd.encoder import LARGE_BATCH_BITS
    if c["bitrate"] is not None:
        monkeypatch.setenv("VBM_WORKSPACES", "2")       # fifteen packetblobs per workspace (as tests/test_full_size_gpu.py)
    stat = lb.run_case(oracle, cuda, c)
    print(f"{c['name']}: R = {stat['R']}, {stat['blocks']} blocks compared with the oracle, {stat['rows']} rows with their twins, "
          f"{stat['calls']} calls, masks " + ", ".join(f"type {m}: {sorted(s)}" for m, s in sorted(stat["masks"].items())))
    assert set(stat["masks"]) == set(lb.block_types(c)), sorted(stat["masks"])
    for mode, masks in stat["masks"].items():
        assert all(m & LARGE_BATCH_BITS == lb.wanted_bits(mode) for m in masks), (mode, sorted(masks))
