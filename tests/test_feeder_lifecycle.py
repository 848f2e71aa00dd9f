"""The prefetch lifecycle every feeder shares (feeder._Prefetcher), driven by trivial producers on the CPU: the device calls of the
worker and of the consumer's loop are replaced by stand-ins, so what is checked is the thread / queue / stop / error handling alone.
Every wait runs in a thread joined with a timeout: a hang fails the test instead of stalling the suite."""
import threading
import time

import pytest
import torch

from himo_amd import feeder

WAIT = 10.0


class _Stream:
    def wait_event(self, ev):
        pass


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())


class _Counter(feeder._Prefetcher):
    """items 0, 1, ... up to ``n`` (forever when None), then ``error`` if one is given; ``hold``: after the items, wait for close()"""

    def __init__(self, n=None, error=None, hold=False, depth=2):
        self.device = "stand-in"
        self.n, self.error, self.hold = n, error, hold
        self.teardowns = 0
        self._start(depth, "himo-test-feeder")

    def _produce(self):
        i = 0
        while self.n is None or i < self.n:
            if not self._offer((i, None, ())):
                return
            i += 1
        if self.error is not None:
            raise self.error
        while self.hold and not self._stop:              # a slow source: nothing more arrives until the feeder is stopped
            time.sleep(0.01)

    def _teardown(self):
        self.teardowns += 1


def _consume(f, got: list, errors: list) -> threading.Thread:
    def run():
        try:
            for x in f:
                got.append(x)
        except BaseException as e:
            errors.append(e)
    t = threading.Thread(target=run, daemon=True)
    t.start()
    return t


def _closed(f):
    assert not f._thread.is_alive()
    assert f.teardowns == 1


def test_a_blocked_consumer_returns_when_another_thread_closes():
    f = _Counter(n=2, hold=True)
    got, errors = [], []
    t = _consume(f, got, errors)
    deadline = time.monotonic() + WAIT
    while len(got) < 2 and time.monotonic() < deadline:
        time.sleep(0.01)
    assert got == [0, 1]                                   # the consumer now waits for an item that never comes
    f.close()
    t.join(timeout=WAIT)
    assert not t.is_alive() and errors == []
    _closed(f)


def test_iterating_after_close_returns_at_once():
    f = _Counter()                                         # an endless source: the worker is blocked on a full queue
    f.close()
    _closed(f)
    got, errors = [], []
    t = _consume(f, got, errors)
    t.join(timeout=WAIT)
    assert not t.is_alive() and got == [] and errors == []


def test_a_producer_error_follows_the_items_before_it():
    f = _Counter(n=3, error=OSError("disk gone"), depth=1)
    got, errors = [], []
    t = _consume(f, got, errors)
    t.join(timeout=WAIT)
    assert not t.is_alive()
    assert got == [0, 1, 2]
    assert len(errors) == 1 and isinstance(errors[0], OSError)


def test_close_twice_and_after_the_end():
    f = _Counter(n=4)
    got, errors = [], []
    t = _consume(f, got, errors)
    t.join(timeout=WAIT)
    assert not t.is_alive() and got == [0, 1, 2, 3] and errors == []
    for _ in range(2):
        closer = threading.Thread(target=f.close, daemon=True)
        closer.start()
        closer.join(timeout=WAIT + 30)
        assert not closer.is_alive()
    _closed(f)


def test_the_device_storages_are_recorded_once_each(monkeypatch):
    """the consumer records every distinct storage of an item on its stream once, whatever number of views of it the item names"""
    recorded = []
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, stream: recorded.append(self.untyped_storage().data_ptr()))
    block, other = torch.zeros(64, dtype=torch.uint8), torch.zeros(8)

    class _Views(feeder._Prefetcher):
        def __init__(self):
            self.device = "stand-in"
            self._start(1, "himo-test-feeder")

        def _produce(self):
            self._offer(("batch", None, [block[:16], block[16:], other, block]))

    got = []
    t = _consume(_Views(), got, [])
    t.join(timeout=WAIT)
    assert not t.is_alive() and got == ["batch"]
    assert recorded == [block.untyped_storage().data_ptr(), other.untyped_storage().data_ptr()]
