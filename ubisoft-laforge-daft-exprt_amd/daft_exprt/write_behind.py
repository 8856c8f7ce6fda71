"""Write-behind stage of the data-set passes (`extract_features.extract_features`, `fine_tune.fine_tuning`).

A pass packs everything a batch writes into one uint8 device buffer; `WriteBehind.put` starts its copy to pinned host memory
and returns, and a thread of the stage's own waits for the copy and hands the bytes to the pass's `write`, so the next
batch's device work never waits for file output.
"""
import queue
import threading
import time

import torch


class WriteBehind(object):
    ''' `write(raw, *rest)` -- raw: the batch's bytes as a uint8 NumPy array -- runs on the thread `name`, one job at a time in the
        order of `put`, at most `depth` jobs behind.  The first exception a job raises is kept: the jobs after it are dropped
        unrun (so a full queue never blocks the producer) and `put` and `close` both re-raise it.
        `busy_s`: seconds spent in `write`, the wait for the copy not counted. '''
    def __init__(self, write, name, depth=4):
        self.write, self.error, self.busy_s = write, None, 0.
        self.q = queue.Queue(maxsize=depth)
        self.thread = threading.Thread(target=self._run, name=name, daemon=True)
        self.thread.start()

    def put(self, buf, *rest):
        ''' buf: uint8 device tensor; its copy to the host is ordered behind the work queued on the current stream '''
        if self.error is not None:
            raise self.error
        host = torch.empty(buf.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(buf, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._enqueue(event, host, *rest)

    def _enqueue(self, event, host, *rest):
        ''' the queue side of `put`: `host` holds the bytes once `event.synchronize()` returns '''
        if self.error is not None:
            raise self.error
        self.q.put((event, host, rest))

    def _run(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            if self.error is None:
                event, host, rest = job
                try:
                    event.synchronize()
                    t0 = time.time()
                    self.write(host.numpy(), *rest)
                    self.busy_s += time.time() - t0
                except Exception as e:        # surfaced by put / close
                    self.error = e

    def close(self):
        self.q.put(None)
        self.thread.join()
        if self.error is not None:
            raise self.error
