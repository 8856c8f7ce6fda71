"""CPU checks of the write-behind stage of the data-set passes (`daft_exprt/write_behind.py`) -- order, the kept first error,
a producer that is never blocked -- and of the one parser of a .markers file's span.  The stage is driven below `put`'s device
copy, through `_enqueue`, with a stand-in event and a plain CPU buffer."""
import threading
import time

import numpy as np
import pytest
import torch

from daft_exprt.write_behind import WriteBehind

JOIN_S = 5.0                                                             # a blocked producer fails the test instead of hanging it
MARKER_LINES = ['0.12\t0.30\t15\tHH\thello\t0\n', '0.30\t0.75\t39\tAH0\thello\t0\n', '0.75\t1.8731\t97\tL\thello\t0\n']


class _Event(object):
    ''' stands in for torch.cuda.Event: the copy is done once `synchronize` returns '''
    def __init__(self):
        self.waited = False

    def synchronize(self):
        self.waited = True


def _job(k):
    return torch.full((8,), k, dtype=torch.uint8)


def _close(stage):
    ''' `stage.close()` under a join timeout; returns what it raised, or None '''
    raised = []

    def close():
        try:
            stage.close()
        except Exception as e:
            raised.append(e)

    closer = threading.Thread(target=close, daemon=True)
    closer.start()
    closer.join(JOIN_S)
    assert not closer.is_alive(), 'close() is blocked'
    assert not stage.thread.is_alive()
    return raised[0] if raised else None


def test_jobs_are_written_in_order_with_their_bytes():
    seen, events = [], [_Event() for _ in range(3)]

    def write(raw, k, tag):
        assert isinstance(raw, np.ndarray) and raw.dtype == np.uint8 and events[k - 1].waited
        assert threading.current_thread().name == 'order_writer'
        time.sleep(0.005)
        seen.append((raw.tobytes(), k, tag))

    stage = WriteBehind(write, 'order_writer')
    assert stage.busy_s == 0.
    for k in (1, 2, 3):
        stage._enqueue(events[k - 1], _job(k), k, f'job{k}')
    assert _close(stage) is None
    assert seen == [(bytes([k] * 8), k, f'job{k}') for k in (1, 2, 3)]
    assert stage.busy_s >= 0.015


def test_first_error_is_kept_and_the_producer_never_blocks():
    written, boom = [], OSError('disk full')

    def write(raw, k):
        if k == 2:
            raise boom
        written.append((k, raw.tobytes()))

    stage = WriteBehind(write, 'failing_writer')
    assert stage.q.maxsize == 4
    stage._enqueue(_Event(), _job(1), 1)
    stage._enqueue(_Event(), _job(2), 2)
    while stage.error is None and stage.thread.is_alive():              # job 2 has failed before job 3 is offered
        time.sleep(0.001)
    raised = []

    def produce():
        for k in (3, 4, 5, 6):
            try:
                stage._enqueue(_Event(), _job(k), k)
            except OSError as e:
                raised.append(e)

    producer = threading.Thread(target=produce, daemon=True)
    producer.start()
    producer.join(JOIN_S)
    assert not producer.is_alive(), 'the producer is blocked behind a writer that has stopped'
    assert raised == [boom] * 4
    with pytest.raises(OSError, match='disk full'):
        stage._enqueue(_Event(), _job(7), 7)
    assert _close(stage) is boom
    assert written == [(1, bytes([1] * 8))]


def test_jobs_queued_behind_a_failing_one_are_dropped_unrun():
    ''' seven jobs are on their way before job 2 fails: 1 and 2 have left the queue, 3 to 6 fill it and the producer waits in
        it with job 7.  The writer keeps taking jobs off the queue, so the producer gets through, and runs none of them '''
    written, gate, boom = [], threading.Event(), ValueError('bad batch')

    def write(raw, k):
        if k == 2:
            gate.wait(JOIN_S)
            raise boom
        written.append(k)

    stage = WriteBehind(write, 'draining_writer')
    raised = []

    def produce():
        for k in range(1, 8):
            try:
                stage._enqueue(_Event(), _job(k), k)
            except ValueError as e:
                raised.append(e)

    producer = threading.Thread(target=produce, daemon=True)
    producer.start()
    while stage.q.qsize() < 4 and producer.is_alive():                  # 1 written, 2 in `write`, 3 to 6 queued: the queue is full
        time.sleep(0.001)
    assert producer.is_alive()                                           # job 7 has no room yet
    gate.set()
    producer.join(JOIN_S)
    assert not producer.is_alive(), 'the producer is blocked on a full queue'
    assert _close(stage) is boom
    assert written == [1] and raised in ([], [boom])                    # job 7 went into the queue, or was offered after the failure


def test_close_without_a_job_returns_at_once():
    stage = WriteBehind(lambda raw: None, 'idle_writer')
    assert _close(stage) is None and stage.busy_s == 0.


def test_marker_span_has_one_parser(tmp_path):
    from daft_exprt.extract_features import _FeatureUtterance, marker_lines_span
    from daft_exprt.fine_tune import markers_span
    path = tmp_path / 'u.markers'
    path.write_text(''.join(MARKER_LINES), encoding='utf-8')
    assert markers_span(str(path)) == marker_lines_span(MARKER_LINES) == (0.12, 1.8731)
    utt = _FeatureUtterance('spk', 'u', MARKER_LINES, 'hello')
    assert (utt.sent_begin, utt.sent_end) == markers_span(str(path))
    assert utt.spans == [[0.12 - 0.12, 0.30 - 0.12], [0.30 - 0.12, 0.75 - 0.12], [0.75 - 0.12, 1.8731 - 0.12]]
