"""Device-built rounds with the transforms ahead of the state waits (csrc/capi_encoder.cpp, device_round_run_graphs): a
batch's spread flags, MDCT and FFT graph runs as soon as the round is forked (the big batch's on the front end's own
stream), its psychoacoustics graph behind the state events of the batches its streams may come from.

The base case is the device-built-rounds case of tests/test_ordering_gpu.py (run_device_rounds, tests/encode_calls.py):
2048 streams, 8 twin signals, 18 writes,
bursts every 12000 samples, two rounds per call, the consumer's stream joins.  Packets through the twin ledger and
against the oracle, and all four block types must have run.  A spin kernel (vbm_debug_set_delay) holds up

  dev_big_transforms    the big batch's transforms: its psychoacoustics (another stream) must wait for them, and so must
                        the front end's buffer shift and the next round's plan (the same stream)
  dev_small_transforms  a small batch's transforms
  both, and dev_big_back  the transforms late while the back half of the big batch before still holds its workspace

and one run fills every scratch buffer with 0xFF between the calls: the transforms may read nothing but the round's
gathered PCM and window flags.  The no-delay case and the two single points again with the fewest workspaces the
device-built rounds take (vbm_encoder_create: VBM_WORKSPACES below 2 counts as 2), where a workspace comes round
again after one call."""
import pytest

from tests.encode_calls import check_oracle, delay, run_device_rounds  # noqa: F401 (delay: fixture)

pytestmark = pytest.mark.gpu

NCHUNKS, PERIOD = 18, 12000
FEWEST_WORKSPACES = "2"


def run(oracle, cuda, monkeypatch, poison=False, workspaces="4"):
    led = run_device_rounds(cuda, monkeypatch, NCHUNKS, PERIOD, poison=poison, workspaces=workspaces)
    check_oracle(led, oracle, NCHUNKS, PERIOD)          # (asserts that all four block types ran)


@pytest.mark.parametrize("points", [("dev_big_transforms",), ("dev_small_transforms",),
                                    ("dev_big_transforms", "dev_small_transforms", "dev_big_back")], ids="+".join)
def test_transforms_held_up(oracle, cuda, monkeypatch, delay, points):
    delay(*points)
    run(oracle, cuda, monkeypatch)


def test_poisoned_scratch(oracle, cuda, monkeypatch):
    run(oracle, cuda, monkeypatch, poison=True)


@pytest.mark.parametrize("points", [(), ("dev_big_transforms",), ("dev_small_transforms",)], ids=lambda p: "+".join(p) or "none")
def test_fewest_workspaces(oracle, cuda, monkeypatch, delay, points):
    if points:
        delay(*points)
    run(oracle, cuda, monkeypatch, workspaces=FEWEST_WORKSPACES)
