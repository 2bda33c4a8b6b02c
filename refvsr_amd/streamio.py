"""Host plumbing of videorun's stream loop (no torch, no GPU call: the CPU suite runs all of it): frames come in through reader threads
and leave through a writer thread, in order, through fixed rings of buffers the caller provides (pinned staging memory in videorun,
plain numpy arrays in the tests).

  * `Run`: what the threads of one run share -- a `stop` event and the FIRST exception of any of them, re-raised on the caller's
    thread by every wait (`check()`);
  * `FrameSource`: one reader thread per input.  It opens the stream itself (a FIFO's open blocks until the producer opens its end),
    announces the header (`header()`), then fills the buffers it is given (`provide`, `give`) through `readinto` and hands
    `(index, buffer)` to a bounded queue (`get()`; None behind the last frame);
  * `next_pair`: the next frame of two sources, or the one-line ValueError of a pair whose lengths differ;
  * `FrameSink`: one writer thread.  `put(buffer)` takes frames in order, the thread writes them through a yuv.Y4MWriter and hands
    the buffers back (`take()`); `put(buffer, length)` writes the first `length` elements only -- the variable-length frames of a
    jpeg.MJPEGWriter.

The two inputs are read CONCURRENTLY, each by its own thread, and a source reads ahead as far as its ring reaches before anybody asks:
a producer that fills one FIFO before it opens the other (a decoder that writes the first LR frames, then opens the reference stream)
finds the first one drained meanwhile and does not deadlock the run, as long as the two streams stay within a ring of each other.
Opening both streams one after the other on one thread would hang there for ever.

Threads are daemons, every queue wait has a timeout (0.1 s slices that look at `stop`), `Run.stop` or the first exception ends all of
them, and a source that delivers nothing for `io_timeout` seconds -- or a sink that takes nothing -- ends the run with a ValueError
instead of hanging it.  A reader blocked inside a read of a descriptor is woken by `stop` (yuv.Y4MStreamReader.stop); one blocked in
a file object that cannot be polled, or in the open of a FIFO nobody writes, is left behind as a daemon after `close()` has waited a
second for it.
"""
import queue
import threading
import time

from .yuv import StreamStopped

SLICE = 0.1             # seconds a wait sleeps before it looks at `stop` and at the run's error again


class Run(object):
    """The `stop` event and the first exception of the threads of one run."""

    def __init__(self):
        self.stop = threading.Event()
        self.error = None
        self._lock = threading.Lock()

    def fail(self, exc):
        with self._lock:
            if self.error is None:
                self.error = exc
        self.stop.set()

    def check(self):
        if self.error is not None:
            raise self.error


def _wait(run, q, timeout, what):
    """q.get() in slices: the run's error if one came up, ValueError(what % timeout) after `timeout` seconds of nothing; (item, seconds
    waited)."""
    t0 = time.time()
    while True:
        run.check()
        try:
            return q.get(timeout=SLICE), time.time() - t0
        except queue.Empty:
            if time.time() - t0 >= timeout:
                run.check()
                raise ValueError(what % timeout)


class FrameSource(object):
    """One input stream behind a reader thread.  open_reader(stop) -> a yuv.Y4MStreamReader (called ON the thread); name: what messages
    call the stream.  header() waits for the stream's header and returns the reader (its attributes; nobody else reads from it);
    provide(buffers) hands the ring over -- as soon as the header is known, so that the thread drains its stream while the other
    one still opens (`ring` buffers: the bound of the queue); get() -> (index, buffer) in order, None behind the last frame (and from
    then on); give(buffer) returns one.  `waited`: the seconds get() and header() spent waiting."""

    def __init__(self, run, open_reader, name, ring, io_timeout=120.0):
        self.run, self.name, self.ring, self.io_timeout = run, name, int(ring), float(io_timeout)
        self.reader = None
        self.waited = 0.0
        self.outstanding = 0                # buffers handed out by get() and not given back
        self._open = open_reader
        self._opened = threading.Event()
        self._free, self._full = queue.Queue(), queue.Queue(self.ring + 1)         # (+ 1: the None behind the last frame)
        self._ended = False
        self.thread = threading.Thread(target=self._work, name='refvsr-read-%s' % name, daemon=True)
        self.thread.start()

    def _work(self):
        run = self.run
        try:
            self.reader = self._open(run.stop)
            self._opened.set()
            index = 0
            while not run.stop.is_set():
                try:
                    buf = self._free.get(timeout=SLICE)
                except queue.Empty:
                    continue
                if not self.reader.readinto(buf):
                    self._full.put_nowait(None)
                    return
                self._full.put_nowait((index, buf))     # (never more than the ring holds: the queue cannot be full)
                index += 1
        except StreamStopped:
            pass
        except BaseException as e:                      # noqa: B902 -- whatever it is, the caller's thread gets it
            run.fail(e)
        finally:
            self._opened.set()

    def header(self):
        t0 = time.time()
        while not self._opened.wait(SLICE):
            self.run.check()
            if time.time() - t0 >= self.io_timeout:
                raise ValueError('%s: no data for %g s' % (self.name, self.io_timeout))
        self.run.check()
        self.waited += time.time() - t0
        return self.reader

    def provide(self, buffers):
        assert len(buffers) == self.ring, 'the ring of %s holds %d buffers' % (self.name, self.ring)
        for b in buffers:
            self._free.put(b)

    def get(self):
        if self._ended:
            return None
        item, dt = _wait(self.run, self._full, self.io_timeout, self.name + ': no data for %g s')
        self.waited += dt
        if item is None:
            self._ended = True
        else:
            self.outstanding += 1
        return item

    def give(self, buf):
        self.outstanding -= 1
        self._free.put(buf)

    def close(self):
        """Ends the thread (the run's stop event is set: close every source and sink of a run together) and closes the reader."""
        self.run.stop.set()
        self.thread.join(1.0)
        if self.reader is not None and not self.thread.is_alive():
            self.reader.close()


def next_pair(a, b, what='videorun'):
    """The next frames of two sources: ((index, buffer a), (index, buffer b)), None when both have ended, ValueError when one has
    ended and the other has not."""
    x, y = a.get(), b.get()
    if x is None and y is None:
        return None
    if x is None or y is None:
        k = (y if x is None else x)[0]
        raise ValueError('%s: %s and %s: frame count differs (%s)' % (
            what, a.name, b.name, '%d and more than %d' % (k, k) if x is None else 'more than %d and %d' % (k, k)))
    return x, y


class FrameSink(object):
    """The output behind a writer thread.  writer: a yuv.Y4MWriter (written to by the thread alone); buffers: the ring.  take() -> a
    free buffer (waits for the writer: `waited`); put(buffer) queues a frame, in order -- put(buffer, length): the frame is
    buffer[:length] (a jpeg.MJPEGWriter's compressed frame in a slot of the ring); put(buffer, data=bytes): the frame is `data`, the
    buffer only returns to the ring in its turn (a frame larger than a slot); finish() waits until everything queued is written.  The writer is not closed here: who opened it closes it."""

    def __init__(self, run, writer, buffers, name, io_timeout=120.0):
        self.run, self.writer, self.name, self.io_timeout = run, writer, name, float(io_timeout)
        self.waited = 0.0
        self.outstanding = 0                # buffers taken and not written yet
        self._free, self._todo = queue.Queue(), queue.Queue()
        for b in buffers:
            self._free.put(b)
        self._end = object()
        self._finished = threading.Event()
        self.thread = threading.Thread(target=self._work, name='refvsr-write-%s' % name, daemon=True)
        self.thread.start()

    def _work(self):
        run = self.run
        try:
            while not run.stop.is_set():
                try:
                    item = self._todo.get(timeout=SLICE)
                except queue.Empty:
                    continue
                if item is self._end:
                    self._finished.set()
                    return
                buf, length, data = item
                self.writer.write(data if data is not None else buf if length is None else buf[:length])
                self._free.put(buf)
        except BaseException as e:                      # noqa: B902
            run.fail(e)

    def take(self):
        buf, dt = _wait(self.run, self._free, self.io_timeout, self.name + ': nothing written for %g s')
        self.waited += dt
        self.outstanding += 1
        return buf

    def put(self, buf, length=None, data=None):
        self.run.check()
        self.outstanding -= 1
        self._todo.put((buf, length, data))

    def finish(self):
        self._todo.put(self._end)
        t0 = time.time()
        mark, since = self.writer.frames, t0
        while not self._finished.wait(SLICE):
            self.run.check()
            if self.writer.frames != mark:
                mark, since = self.writer.frames, time.time()
            if time.time() - since >= self.io_timeout:
                raise ValueError('%s: nothing written for %g s' % (self.name, self.io_timeout))
        self.run.check()
        self.waited += time.time() - t0

    def close(self):
        self.run.stop.set()
        self.thread.join(1.0)
