"""CPU: KernelTimer's selection over hand-built ConvRecords (no events, no GPU): collect / collect_bytes
filter by the x3 flag and by family, and a ConvRecord is still the 8-tuple bench.py and the scripts read
by position."""
from fastvideocodec_amd import profiling
from fastvideocodec_amd.profiling import ConvRecord


def _timer():
    t = profiling.KernelTimer()
    t.records += [
        ConvRecord(None, None, 10.0, "a x3", True, 100, "x3", 2),
        ConvRecord(None, None, 20.0, "b wino", True, 200, "wino", 1),
        ConvRecord(None, None, 40.0, "b wino x4", True, 400, "wino", 4),
        ConvRecord(None, None, 80.0, "c", False, 800, "f32", 1),
        ConvRecord(None, None, 160.0, "d dx", True, 1600, "dx", 1),
    ]
    return t


def test_field_order():
    assert ConvRecord._fields == ("ev0", "ev1", "flops", "key", "x3", "nbytes", "family", "dispatches")
    r = ConvRecord("e0", "e1", 1.0, "k", True, 7, "stem", 3)
    assert tuple(r) == ("e0", "e1", 1.0, "k", True, 7, "stem", 3)
    assert (r[2], r[3], r[4], r[5], r[6], r[7]) == (r.flops, r.key, r.x3, r.nbytes, r.family, r.dispatches)


def test_select_by_x3_and_family():
    t = _timer()
    keys = lambda rs: [r.key for r in rs]  # noqa: E731
    assert keys(t._select(None, None)) == ["a x3", "b wino", "b wino x4", "c", "d dx"]
    assert keys(t._select(True, None)) == ["a x3", "b wino", "b wino x4", "d dx"]
    assert keys(t._select(False, None)) == ["c"]
    assert keys(t._select(None, "wino")) == ["b wino", "b wino x4"]
    assert keys(t._select(True, "x3")) == ["a x3"]
    assert keys(t._select(True, "f32")) == [] and keys(t._select(False, "f32")) == ["c"]
    assert keys(t._select(None, "stem")) == []


def test_collect_bytes_by_x3_and_family():
    t = _timer()
    assert t.collect_bytes() == 3100
    assert t.collect_bytes(x3=True) == 2300
    assert t.collect_bytes(x3=False) == 800
    assert t.collect_bytes(x3=True, family="wino") == 600
    assert t.collect_bytes(family="dx") == 1600
    assert t.collect_bytes(x3=False, family="wino") == 0


def test_timed_conv_untimed_path_describes_nothing():
    """With no timer active the helper runs the launch and nothing else: the description is not evaluated."""
    def describe():
        raise AssertionError("described without a timer")
    assert profiling.active() is None
    assert profiling.timed_conv(lambda: 5, describe) == 5
