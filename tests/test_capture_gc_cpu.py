"""The guard that keeps Python's cyclic garbage collector out of stream captures (randlanet/_train.py: _no_collection): no
cycle is finalised inside the block, and the collector's state is what it was afterwards."""
import gc


class _Cycle:
    def __init__(self, log, name):
        self.me, self.log, self.name = self, log, name

    def __del__(self):
        self.log.append(self.name)


def test_nothing_is_collected_inside():
    from randlanet._train import _no_collection
    log = []
    assert gc.isenabled()
    gc.collect()
    _Cycle(log, "before")                            # dead at once, but a cycle: only a collection finalises it
    assert log == []
    with _no_collection():
        assert not gc.isenabled()
        _Cycle(log, "inside")
        for _ in range(3 * gc.get_threshold()[0]):   # allocations that would set an automatic collection off
            _Cycle([], "other")
        assert log == []
    assert gc.isenabled()
    gc.collect()
    assert sorted(log) == ["before", "inside"]


def test_leaves_a_disabled_collector_disabled_and_survives_an_exception():
    from randlanet._train import _no_collection
    gc.disable()
    try:
        with _no_collection():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
    try:
        with _no_collection():
            raise KeyError("x")
    except KeyError:
        pass
    assert gc.isenabled()
