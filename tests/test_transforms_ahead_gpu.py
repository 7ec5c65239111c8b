"""Device-built rounds with the transforms ahead of the state waits (csrc/capi_encoder.cpp, device_round_run_graphs): a
batch's spread flags, MDCT and FFT graph runs as soon as the round is forked (the big batch's on the front end's own
stream), its psychoacoustics graph behind the state events of the batches its streams may come from.

The base case is the device-built-rounds case of tests/test_ordering_gpu.py: 2048 streams, 8 twin signals, 18 writes,
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

from tests import test_ordering_gpu as og

pytestmark = pytest.mark.gpu

NCHUNKS, PERIOD = 18, 12000
POINTS = dict(og.POINTS, dev_big_transforms=16, dev_small_transforms=17)      # csrc/vbm_internal.h, enum vbm_delay_point
FEWEST_WORKSPACES = "2"


@pytest.fixture
def delay():
    import vorbis_aotuv_lancer_amd as v

    def set_points(*names):
        mask = 0
        for n in names:
            mask |= 1 << POINTS[n]
        assert v.lib.vbm_debug_set_delay(mask, og.DELAY_US if mask else 0) == 0
    yield set_points
    v.lib.vbm_debug_set_delay(0, 0)


class Env:
    """monkeypatch for run_device_rounds, which sets VBM_WORKSPACES itself: with `workspaces` that value instead"""

    def __init__(self, monkeypatch, workspaces):
        self.monkeypatch, self.workspaces = monkeypatch, workspaces

    def setenv(self, name, value):
        self.monkeypatch.setenv(name, self.workspaces if name == "VBM_WORKSPACES" and self.workspaces else value)


def run(oracle, cuda, monkeypatch, poison=False, workspaces=None):
    led = og.run_device_rounds(cuda, Env(monkeypatch, workspaces), NCHUNKS, PERIOD, poison=poison)
    og.check_oracle(led, oracle, NCHUNKS, PERIOD)          # (asserts that all four block types ran)


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
