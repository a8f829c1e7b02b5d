"""The host pieces every recorder shares (knpemi.recording): the tap of a stepper and the row series, driven by stub
`record` / `read` callables.  No library is loaded."""
import numpy as np
import pytest

from knpemi.recording import RowSeries, Tap

GDIM = 3


class Series(RowSeries):
    """Two columns of width 1 around one of width gdim."""

    def __init__(self):
        self._init_series()

    def columns(self):
        return [("a", 1), ("v", GDIM), ("b", 1)]


class Device:
    """What a tap sees of the device: a buffer of `capacity` rows with the two counters of a series buffer.  Row i of a
    series is [t, t + 1, ..., t + n_cols - 1] of its own time stamp."""

    def __init__(self, capacity, n_cols, extra_rows=0):
        self.capacity, self.n_cols, self.extra_rows = capacity, n_cols, extra_rows
        self.rows, self.dropped = [], 0
        self.calls = []                   # (t, fields) of every record
        self.reads = self.rewinds = 0

    def record(self, t, fields):
        self.calls.append((t, fields))
        if len(self.rows) < self.capacity:
            self.rows.append(t + np.arange(self.n_cols))
        else:
            self.dropped += 1

    def read(self, n, buf):
        self.reads += 1
        k = min(n, len(self.rows))
        if k:
            buf[:k] = self.rows[:k]
        out = (len(self.rows) + self.extra_rows, self.dropped)
        self.rows, self.dropped = [], 0
        return out

    def rewind(self):
        self.rewinds += 1
        self.rows, self.dropped = [], 0


def _tap(dev, every=1, offset=0, capacity=None, t0=0.0, fields=False):
    target = Series()
    return target, Tap(target, "stub", every, dev.record, t0, offset=offset, capacity=capacity or dev.capacity,
                       read=dev.read, n_cols=dev.n_cols, rewind=dev.rewind, fields=fields)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("every", [1, 2, 3])
def test_schedule_and_time_stamps(every, offset):
    """End of step (offset 0): the stepper ticks with k = 1, 2, ...; inside the step (offset 1): with k = 0, 1, ...  Either
    way the rows are those of the steps whose number from 1 is a multiple of `every`, stamped with the step's end."""
    dt, t0, steps = 0.125, 0.25, 7
    dev = Device(64, 5)
    target, tap = _tap(dev, every, offset, t0=t0)
    for step in range(steps):
        tap.tick(step + 1 - offset, dt)
    due = [n for n in range(1, steps + 1) if n % every == 0]
    want = [t0 + n * dt for n in due]
    assert [t for t, _ in dev.calls] == want and tap.pending == want
    ser = target.series()
    assert np.array_equal(ser["t"], want) and tap.pending == []


def test_series_splits_columns_of_width_one_and_gdim():
    dev = Device(8, 2 + GDIM)
    target, tap = _tap(dev)
    for k in (1, 2, 3):
        tap.tick(k, 1.0)
    ser = target.series()
    assert set(ser) == {"t", "a", "v", "b"}
    assert ser["a"].shape == (3,) and ser["v"].shape == (3, GDIM) and ser["b"].shape == (3,)
    t = np.array([1.0, 2.0, 3.0])
    assert np.array_equal(ser["a"], t) and np.array_equal(ser["b"], t + 1 + GDIM)
    assert np.array_equal(ser["v"], t[:, None] + 1 + np.arange(GDIM))
    # the flat row of a row dictionary, in the same order
    row = dict(b=9.0, v=np.array([2.0, 3.0, 4.0]), a=1.0)
    assert np.array_equal(target.row_vector(row), [1.0, 2.0, 3.0, 4.0, 9.0])
    # an empty series keeps its shapes
    target.clear()
    empty = target.series()
    assert empty["t"].shape == (0,) and empty["a"].shape == (0,) and empty["v"].shape == (0, GDIM)


def test_drains_exactly_at_capacity_and_at_series():
    dev = Device(3, 5)
    target, tap = _tap(dev)
    for k in (1, 2):
        tap.tick(k, 1.0)
    assert dev.reads == 0 and len(tap.pending) == 2 and target._t == []
    tap.tick(3, 1.0)                      # the buffer holds `capacity` rows: drained
    assert dev.reads == 1 and tap.pending == [] and target._t == [1.0, 2.0, 3.0] and dev.rows == []
    tap.tick(4, 1.0)
    assert dev.reads == 1 and tap.pending == [4.0]
    ser = target.series()                 # drains what is left
    assert dev.reads == 2 and tap.pending == [] and np.array_equal(ser["t"], [1.0, 2.0, 3.0, 4.0])
    assert np.array_equal(ser["a"], ser["t"])
    target.series()                       # nothing pending: the device reports 0 rows, the series is unchanged
    assert dev.reads == 3 and target._t == [1.0, 2.0, 3.0, 4.0]


def test_row_count_mismatch_and_dropped_rows_raise():
    dev = Device(4, 5, extra_rows=1)      # the device reports a row the host did not enqueue
    target, tap = _tap(dev)
    tap.tick(1, 1.0)
    with pytest.raises(RuntimeError, match=r"stub: the device holds 2 row\(s\) \(\+0 dropped\), the host enqueued 1"):
        target.series()
    dev = Device(2, 5)                    # the host believes in more room than the device has: a row is dropped
    target, tap = _tap(dev, capacity=4)
    for k in (1, 2, 3):
        tap.tick(k, 1.0)
    with pytest.raises(RuntimeError, match=r"stub: the device holds 2 row\(s\) \(\+1 dropped\), the host enqueued 3"):
        target.series()


def test_reset_empties_pending_and_series():
    dev = Device(2, 5)
    target, tap = _tap(dev)
    for k in (1, 2, 3):
        tap.tick(k, 1.0)
    assert target._t == [1.0, 2.0] and tap.pending == [3.0]
    tap.reset()
    assert dev.rewinds == 1 and tap.pending == [] and target._t == [] and target._rows == []
    assert target.series()["t"].shape == (0,)
    tap.tick(1, 1.0)
    assert np.array_equal(target.series()["t"], [1.0])


def test_disabled_tap_makes_no_call_and_fields_flag_is_passed():
    dev = Device(8, 5)
    target, tap = _tap(dev, fields=True)
    tap.enabled = False
    for k in (1, 2):
        tap.tick(k, 1.0)
    assert dev.calls == [] and dev.reads == 0 and tap.pending == []
    tap.enabled = True
    tap.tick(3, 1.0)
    tap.fields = False
    tap.tick(4, 1.0)
    assert dev.calls == [(3.0, 1), (4.0, 0)]
    assert np.array_equal(target.series()["t"], [3.0, 4.0])


def test_a_tap_without_a_series_only_records():
    """The membrane events: a record per due step with its time, nothing pending, nothing drained."""
    calls, rewinds = [], []
    target = object()
    tap = Tap(target, "events", 2, lambda t, fields: calls.append(t), t0=1.0, rewind=lambda: rewinds.append(1))
    for k in range(1, 6):
        tap.tick(k, 0.5)
    assert calls == [2.0, 3.0] and tap.pending == []
    tap.reset()
    assert rewinds == [1]
