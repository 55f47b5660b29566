"""The sync-free decision of render_train (render._SyncFreeDecision) without a GPU: the object is driven with a plain tensor in the
place of its pinned buffer and an event whose query() the test controls.  The GPU check of the same rules on a renderer is
tests/test_train_gpu.py::test_render_train_falls_back_to_compaction_when_rays_miss."""
import importlib

import pytest
import torch

render = importlib.import_module("tetra-nerf_amd.render")


class Event:
    """stands in for torch.cuda.Event: the copy has landed when the test says so"""

    def __init__(self):
        self.landed, self.recorded = False, 0

    def record(self, stream=None):
        self.recorded += 1

    def query(self):
        return self.landed


@pytest.fixture
def decision():
    d = render._SyncFreeDecision()
    d.pinned, d.event = torch.zeros(1, dtype=torch.int32), Event()
    return d


def count(n):
    return torch.tensor([n], dtype=torch.int32)


def test_a_fresh_renderer_starts_sync_free(decision):
    assert decision.fraction == 1.0
    assert decision.begin_batch(0.85) is True


def test_landed_copy_gives_count_over_rays(decision):
    d = decision
    assert d.begin_batch(0.85)
    d.start_copy(count(300), 400, None)
    assert d.event.recorded == 1 and int(d.pinned[0]) == 300
    assert d.fraction == 1.0                     # nothing is read before a batch starts
    assert d.begin_batch(0.85)                   # ... and nothing before the copy has landed
    assert d.fraction == 1.0 and d.pending is not None
    d.event.landed = True
    assert d.begin_batch(0.85) is False          # 300 / 400 < 0.85
    assert d.fraction == 0.75 and d.pending is None


def test_fraction_of_an_empty_batch_divides_by_one(decision):
    d = decision
    d.begin_batch(0.85)
    d.start_copy(count(0), 0, None)
    d.event.landed = True
    d.begin_batch(0.85)
    assert d.fraction == 0.0                     # count / max(rays, 1)
    d.host_counted(0, 0)
    assert d.fraction == 0.0


def test_no_second_copy_while_one_is_pending(decision):
    d = decision
    d.begin_batch(0.85)
    d.start_copy(count(100), 100, None)
    d.begin_batch(0.85)
    d.start_copy(count(7), 100, None)            # the buffer is busy: this batch's count is not copied
    assert d.event.recorded == 1 and int(d.pinned[0]) == 100 and d.pending == (1, 100)
    d.event.landed = True
    assert d.begin_batch(0.85) and d.fraction == 1.0
    d.event.landed = False
    d.start_copy(count(7), 100, None)            # free again
    assert d.event.recorded == 2 and int(d.pinned[0]) == 7 and d.pending == (3, 100)


def test_read_back_that_lands_after_a_newer_host_count_is_ignored(decision):
    d = decision
    d.begin_batch(0.85)                          # batch 1: sync-free, all of its rays hit
    d.start_copy(count(100), 100, None)
    d.begin_batch(0.85)                          # batch 2: compacting (a call with capture=, say): the host sees half of them miss
    d.host_counted(50, 100)
    assert d.fraction == 0.5
    d.event.landed = True                        # batch 1's copy lands now
    assert d.begin_batch(0.85) is False          # batch 3 decides on batch 2's fraction
    assert d.fraction == 0.5 and d.pending is None
    # the other order: a copy issued AFTER the host count does override it
    d.event.landed = False
    d.start_copy(count(90), 100, None)           # (as batch 3, had it been sync-free)
    d.event.landed = True
    assert d.begin_batch(0.85) is True and d.fraction == 0.9


@pytest.mark.parametrize("hits,allowed", [(84, False), (85, True), (86, True)])
def test_decision_is_last_known_fraction_at_least_the_threshold(decision, hits, allowed):
    d = decision
    d.begin_batch(0.85)
    d.host_counted(hits, 100)
    assert d.fraction == hits / 100
    assert d.begin_batch(hits / 100) is True     # >=: equality allows the sync-free form
    assert d.begin_batch(0.85) is allowed
    assert d.begin_batch(0.0) is True


def test_renderer_exposes_the_fraction():
    rd = render.TetraRenderer.__new__(render.TetraRenderer)
    rd._sync_free = render._SyncFreeDecision()
    rd._sync_free.host_counted(1, 4)
    assert rd._hit_fraction == 0.25
