"""videorun's stream loop, the host side (no GPU): yuv.Y4MStreamReader on pipes that deliver a byte at a time, the Y4MWriter ->
pipe -> reader round trip, scene.GroupPlanner for a length nobody knows (every case against scene.plan_groups), streamio's reader and
writer threads -- order, recycling, the four ways a run ends in an error, no thread left behind -- and the new options."""
import io
import itertools
import os
import threading
import time

import numpy as np
import pytest

from refvsr_amd import scene, streamio, yuv

PLANAR = ('i420', 'i420p10', 'i422', 'i422p10', 'i444', 'i444p10')
# the eight planar forms a header can name: the six samplings x depths, and the two 4:2:0 sitings a tag says (C420mpeg2, XCHROMASITING)
FORMS = tuple((f, None) for f in PLANAR) + (('i420', 'left'), ('i420p10', 'left'))
H, W = 6, 10


def frames_of(fmt, n, seed=3):
    rs = np.random.RandomState(seed + len(fmt))
    top = 256 if yuv.depth_of(fmt) == 8 else 1024
    return [rs.randint(0, top, yuv.frame_shape(H, W, fmt)).astype(yuv.dtype_of(fmt)) for _ in range(n)]


def file_bytes(tmp_path, fmt, frames, siting=None, name='a.y4m'):
    path = str(tmp_path / name)
    with yuv.Y4MWriter(path, H, W, fmt, (25, 1), 'full', siting) as wr:
        for f in frames:
            wr.write(f)
    return path, open(path, 'rb').read()


def feed(data, chunk, close=True):
    """An os.pipe() whose write end a daemon thread feeds `data` in writes of `chunk` bytes; the read end as an unbuffered file."""
    r, w = os.pipe()

    def work():
        try:
            for i in range(0, len(data), chunk):
                os.write(w, data[i:i + chunk])
        except OSError:
            pass
        finally:
            if close:
                os.close(w)
    th = threading.Thread(target=work, daemon=True)
    th.start()
    return os.fdopen(r, 'rb', buffering=0), th


def settle(start, seconds=5.0):
    """threading.active_count() is back at `start` within `seconds`."""
    t0 = time.time()
    while threading.active_count() > start and time.time() - t0 < seconds:
        time.sleep(0.02)
    assert threading.active_count() <= start, [t.name for t in threading.enumerate()]


# ------------------------------------------------------------------------------------------------ Y4MStreamReader
@pytest.mark.parametrize('chunk', [1, 4093])
@pytest.mark.parametrize('fmt, siting', FORMS)
def test_stream_reader_on_a_pipe_gives_the_files_frames(tmp_path, fmt, siting, chunk):
    frames = frames_of(fmt, 3)
    path, data = file_bytes(tmp_path, fmt, frames, siting)
    with yuv.Y4MReader(path) as rd:
        want = list(rd)
        attrs = (rd.h, rd.w, rd.fps, rd.fmt, rd.range, rd.siting)
    assert len(want) == 3
    fh, th = feed(data, chunk)
    with fh, yuv.Y4MStreamReader(fh) as sr:
        assert sr.length is None and yuv.Y4MStreamReader.length is None
        assert (sr.h, sr.w, sr.fps, sr.fmt, sr.range, sr.siting) == attrs
        got = [sr.read()]
        buf = np.empty(yuv.frame_shape(H, W, fmt), yuv.dtype_of(fmt))
        assert sr.readinto(buf) is True
        got.append(buf.copy())
        got.append(sr.read())
        assert sr.frames == 3 and sr.read() is None and sr.readinto(buf) is False
    th.join(5)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_stream_reader_sources(tmp_path):
    """A path, a buffered file object, an object that knows neither seek nor fileno and hands out three bytes at a time."""
    frames = frames_of('i420', 2)
    path, data = file_bytes(tmp_path, 'i420', frames)

    class Drip(object):
        def __init__(self, data):
            self.data, self.pos = data, 0

        def read(self, n=-1):
            k = min(3, n) if n >= 0 else 3
            out = self.data[self.pos:self.pos + k]
            self.pos += len(out)
            return out

        def seek(self, *a):
            raise io.UnsupportedOperation('seek')

        def fileno(self):
            raise io.UnsupportedOperation('fileno')
    for src in (path, open(path, 'rb'), io.BytesIO(data), Drip(data)):
        with yuv.Y4MStreamReader(src) as sr:
            got = list(sr)
        assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, frames))
        if hasattr(src, 'closed'):
            assert not src.closed                        # only what the reader opened is closed by it
            src.close()


def test_stream_reader_markers_and_truncation(tmp_path):
    frames = frames_of('i420', 3)
    _, data = file_bytes(tmp_path, 'i420', frames)
    nb = yuv.frame_bytes(H, W, 'i420')
    head = data[:data.index(b'\n') + 1]
    body = [data[len(head) + k * (6 + nb) + 6:len(head) + (k + 1) * (6 + nb)] for k in range(3)]
    # FRAME with parameters is a frame marker
    with yuv.Y4MStreamReader(io.BytesIO(head + b'FRAME Ip\n' + body[0] + b'FRAME Ip XFOO=1\n' + body[1] + b'FRAME\n' + body[2])) as sr:
        got = list(sr)
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, frames))
    # a truncated last frame is reported by index, the whole frames before it are delivered
    for cut in (1, nb // 2, nb - 1):
        sr = yuv.Y4MStreamReader(io.BytesIO(data[:len(data) - cut]))
        assert np.array_equal(sr.read(), frames[0]) and np.array_equal(sr.read(), frames[1])
        with pytest.raises(ValueError, match=r'BytesIO.*: truncated frame 2$'):
            sr.read()
    # bad markers: the existing message
    for bad in (b'FRAMF\n' + body[1], b'FRAMEX\n' + body[1], b'FRA', b'FRAME ' + b'x' * 100 + b'\n' + body[1], b'FRAME Ip'):
        sr = yuv.Y4MStreamReader(io.BytesIO(head + b'FRAME\n' + body[0] + bad))
        assert sr.read() is not None
        with pytest.raises(ValueError, match=r'FRAME marker expected before frame 1$'):
            sr.read()
    # the header: parse_y4m_header's refusals, in its words
    for hd, text in ((b'YUV4MPEG2 W10 H6 F25:1 It\n', 'interlaced file'), (b'YUV4MPEG2 W10 H6 F25:1 C420paldv\n', 'top-left sited chroma'),
                     (b'YUV4MPEG2 W10 H6 F25:1 Cmono\n', 'no chroma'), (b'RIFF W10 H6\n', 'not a YUV4MPEG2 file'), (b'YUV4MPEG2 W10 H6', 'not a YUV4MPEG2 file'),
                     (b'YUV4MPEG2 W11 H6 F25:1\n', 'even, positive')):
        with pytest.raises(ValueError, match=text):
            yuv.Y4MStreamReader(io.BytesIO(hd))
    # readinto: only the frame's own shape and dtype, contiguous and writable
    sr = yuv.Y4MStreamReader(io.BytesIO(data))
    shape = yuv.frame_shape(H, W, 'i420')
    ro = np.empty(shape, np.uint8)
    ro.setflags(write=False)
    for buf in (np.empty(shape, np.uint16), np.empty((shape[0] + 1, shape[1]), np.uint8), np.empty((shape[1], shape[0]), np.uint8).T,
                np.empty(shape[0] * shape[1], np.uint8), ro, bytearray(shape[0] * shape[1])):
        with pytest.raises(ValueError, match='readinto needs a writable, contiguous uint8 array'):
            sr.readinto(buf)
    assert sr.frames == 0 and np.array_equal(sr.read(), frames[0])          # a refused buffer took nothing from the stream


def test_stream_reader_stop_event_ends_a_wait():
    r, w = os.pipe()
    try:
        os.write(w, b'YUV4MPEG2 W10 H6 F25:1\nFRAME\n' + b'\0' * 10)        # a frame that never completes
        stop = threading.Event()
        with os.fdopen(r, 'rb', buffering=0) as fh:
            sr = yuv.Y4MStreamReader(fh, stop)
            threading.Timer(0.2, stop.set).start()
            t0 = time.time()
            with pytest.raises(yuv.StreamStopped):
                sr.read()
            assert time.time() - t0 < 3
    finally:
        os.close(w)


@pytest.mark.parametrize('fmt, siting', FORMS)
def test_writer_pipe_reader_round_trip(tmp_path, fmt, siting):
    frames = frames_of(fmt, 3)
    _, data = file_bytes(tmp_path, fmt, frames, siting)
    r, w = os.pipe()
    got = []

    def read():
        with os.fdopen(r, 'rb', buffering=0) as fh, yuv.Y4MStreamReader(fh) as sr:
            got.extend(sr)
            got.append((sr.fmt, sr.siting, sr.range, sr.fps))
    th = threading.Thread(target=read, daemon=True)
    th.start()
    fw = os.fdopen(w, 'wb')
    wr = yuv.Y4MWriter(fw, H, W, fmt, (25, 1), 'full', siting)
    for f in frames:
        wr.write(f)
    wr.close()
    assert not fw.closed                                 # the writer closes only what it opened ...
    fw.close()
    th.join(5)
    assert not th.is_alive() and len(got) == 4           # ... and had flushed: the reader saw everything once the pipe closed
    assert got[3] == (fmt, yuv.effective_siting(fmt, siting or yuv.Y4M_DEFAULT_SITING[yuv.sampling_of(fmt)]), 'full', (25, 1))
    sink = io.BytesIO()
    with yuv.Y4MWriter(sink, H, W, fmt, (25, 1), 'full', siting) as wr:
        for f in got[:3]:
            wr.write(f)
    assert sink.getvalue() == data                       # the same bytes as the file written by path


def test_writer_reports_a_closed_pipe_in_one_line():
    r, w = os.pipe()
    os.close(r)
    with os.fdopen(w, 'wb', buffering=0) as fw:
        with pytest.raises(ValueError) as e:
            wr = yuv.Y4MWriter(fw, H, W, 'i420')
            wr.write(frames_of('i420', 1)[0])
        assert 'closed the pipe' in str(e.value) and '\n' not in str(e.value) and str(w) in str(e.value)


# ------------------------------------------------------------------------------------------------ GroupPlanner(None, ...)
def cases():
    for n in range(1, 13):
        cutsets = [c for r in range(n) for c in itertools.combinations(range(1, n), r)] if n <= 8 else [(), (1,), (n - 1,), tuple(range(2, n, 3))]
        for t in (3, 5, 7):
            for G in (1, 2, 3, 4):
                for cuts in cutsets:
                    yield n, t, G, cuts


def test_group_planner_with_unknown_length_gives_plan_groups():
    count = 0
    for n, t, G, cuts in cases():
        want = scene.plan_groups(n, t, G, cuts)
        p = scene.GroupPlanner(None, t, G)
        got, f0 = [], 0
        assert p.pop() is None and not p.done()
        for k in range(n):
            p.push(k in cuts)
            while True:
                assert p.need() == f0 + G + t // 2 and not p.done()
                ready = p.known >= p.need()
                g = p.pop()
                assert (g is not None) == ready, 'a group is popped as soon as need() frames are classified, and no sooner'
                if g is None:
                    break
                assert max(i for w_ in g[1] for i in w_) < p.known      # a window reads classified frames only
                got.append(g)
                f0 = g[0][-1] + 1
        p.finish()
        assert p.n == n
        while not p.done():
            assert p.need() <= f0 + G + t // 2
            g = p.pop()
            assert g is not None, 'finish() drains the remaining groups'
            got.append(g)
            f0 = g[0][-1] + 1
        assert p.pop() is None and got == want, (n, t, G, cuts)
        with pytest.raises(ValueError, match='all %d frames are classified' % n):
            p.push(False)
        # with n given: as before
        q = scene.GroupPlanner(n, t, G)
        seen = []
        for k in range(n):
            q.push(k in cuts)
            g = q.pop()
            while g is not None:
                seen.append(g)
                g = q.pop()
        q.finish()
        assert seen == want and q.done() and q.n == n
        count += 1
    assert count > 3000


# ------------------------------------------------------------------------------------------------ streamio
def stream_bytes(fmt, frames, siting=None):
    sink = io.BytesIO()
    with yuv.Y4MWriter(sink, H, W, fmt, (25, 1), 'limited', siting) as wr:
        for f in frames:
            wr.write(f)
    return sink.getvalue()


def ring_of(fmt, n):
    return [np.empty(yuv.frame_shape(H, W, fmt), yuv.dtype_of(fmt)) for _ in range(n)]


def source(run, data, name, ring, timeout=10.0, chunk=4093, close=True):
    fh, th = feed(data, chunk, close)
    src = streamio.FrameSource(run, lambda stop: yuv.Y4MStreamReader(fh, stop), name, ring, timeout)
    return src, fh


def test_streamio_keeps_order_and_recycles_the_rings():
    start = threading.active_count()
    n, ring, fmt = 23, 3, 'i420p10'
    la, lb = frames_of(fmt, n, 5), frames_of(fmt, n, 6)
    run = streamio.Run()
    a, fa = source(run, stream_bytes(fmt, la), 'lr', ring, chunk=1)
    b, fb = source(run, stream_bytes(fmt, lb), 'ref', ring)
    out = io.BytesIO()
    wr = yuv.Y4MWriter(out, H, W, fmt, (25, 1), 'limited')
    sink_ring = ring_of(fmt, 2)
    sink = streamio.FrameSink(run, wr, sink_ring, 'out')
    try:
        assert (a.header().fmt, b.header().fmt) == (fmt, fmt)
        rings = ring_of(fmt, ring), ring_of(fmt, ring)
        a.provide(rings[0])
        b.provide(rings[1])
        ids = [set(id(x) for x in r) for r in rings + (sink_ring,)]
        k = 0
        while True:
            pair = streamio.next_pair(a, b)
            if pair is None:
                break
            (ia, xa), (ib, xb) = pair
            assert ia == ib == k and id(xa) in ids[0] and id(xb) in ids[1]           # in order, in the caller's buffers
            assert np.array_equal(xa, la[k]) and np.array_equal(xb, lb[k])
            assert a.outstanding == b.outstanding == 1
            o = sink.take()
            assert id(o) in ids[2] and sink.outstanding == 1
            o[...] = xa ^ xb
            sink.put(o)
            a.give(xa)
            b.give(xb)
            k += 1
        assert k == n and streamio.next_pair(a, b) is None
        sink.finish()
        assert wr.frames == n and a.outstanding == b.outstanding == sink.outstanding == 0
    finally:
        for x in (a, b, sink):
            x.close()
        fa.close(), fb.close()
    wr.close()
    assert out.getvalue() == stream_bytes(fmt, [x ^ y for x, y in zip(la, lb)])
    settle(start)


def test_streamio_reads_ahead_no_further_than_the_ring():
    start = threading.active_count()
    fmt, ring = 'i420', 4
    run = streamio.Run()
    a, fa = source(run, stream_bytes(fmt, frames_of(fmt, 9)), 'lr', ring)
    try:
        a.header()
        a.provide(ring_of(fmt, ring))
        t0 = time.time()
        while a.reader.frames < ring and time.time() - t0 < 5:
            time.sleep(0.01)
        time.sleep(0.05)
        assert a.reader.frames == ring                   # the ring is full: the thread waits for a buffer, the stream for the thread
        got = [a.get() for _ in range(ring)]
        assert [g[0] for g in got] == list(range(ring)) and a.outstanding == ring
        with pytest.raises(AssertionError):
            a.provide(ring_of(fmt, ring + 1))
    finally:
        a.close()
        fa.close()
    settle(start)


def test_streamio_unequal_lengths():
    start = threading.active_count()
    fmt = 'i420'
    for na, nb, text in ((4, 3, r'videorun: lr and ref: frame count differs \(more than 3 and 3\)'),
                         (2, 5, r'videorun: lr and ref: frame count differs \(2 and more than 2\)')):
        run = streamio.Run()
        a, fa = source(run, stream_bytes(fmt, frames_of(fmt, na)), 'lr', 2)
        b, fb = source(run, stream_bytes(fmt, frames_of(fmt, nb)), 'ref', 2)
        try:
            a.header(), b.header()
            a.provide(ring_of(fmt, 2)), b.provide(ring_of(fmt, 2))
            with pytest.raises(ValueError, match=text):
                while True:
                    (_, xa), (_, xb) = streamio.next_pair(a, b)
                    a.give(xa), b.give(xb)
        finally:
            a.close(), b.close()
            fa.close(), fb.close()
        settle(start)


def test_streamio_a_silent_source_ends_the_run():
    start = threading.active_count()
    fmt = 'i420'
    data = stream_bytes(fmt, frames_of(fmt, 2))
    for cut, where in ((5, 'header'), (len(data) - 7, 'frames')):            # silent before the header is complete | inside frame 1
        run = streamio.Run()
        a, fa = source(run, data[:cut], 'lr', 2, timeout=0.5, close=False)   # (the write end stays open: nothing comes, no end either)
        try:
            t0 = time.time()
            with pytest.raises(ValueError, match=r'^lr: no data for 0\.5 s$'):
                a.header()
                a.provide(ring_of(fmt, 2))
                assert a.get()[0] == 0
                a.get()
            assert 0.4 < time.time() - t0 < 3, where
        finally:
            a.close()
            fa.close()
        settle(start)


def test_streamio_errors_of_the_threads_reach_the_caller():
    start = threading.active_count()
    fmt = 'i420'
    frames = frames_of(fmt, 6)
    data = stream_bytes(fmt, frames)

    class Boom(object):
        def __init__(self, after, exc):
            self.after, self.exc, self.frames = after, exc, 0

        def write(self, buf):
            if self.frames == self.after:
                raise self.exc
            self.frames += 1
    r, w = os.pipe()
    os.close(r)
    gone = os.fdopen(w, 'wb', buffering=0)

    def broken():
        wr = yuv.Y4MWriter(io.BytesIO(), H, W, fmt)
        wr.fh, wr.name = gone, 'encoder'                  # the pipe's reader goes away behind the header
        return wr
    for make, text in ((lambda: Boom(2, RuntimeError('disk full')), 'disk full'), (broken, r'^encoder: the sink closed the pipe behind frame 0$')):
        run = streamio.Run()
        a, fa = source(run, data, 'lr', 2)
        sink = streamio.FrameSink(run, make(), ring_of(fmt, 2), 'out')
        try:
            a.header()
            a.provide(ring_of(fmt, 2))
            with pytest.raises((RuntimeError, ValueError), match=text):
                while True:
                    item = a.get()
                    if item is None:
                        break
                    o = sink.take()
                    o[...] = item[1]
                    a.give(item[1])
                    sink.put(o)
                sink.finish()
            assert run.stop.is_set()                      # the first exception ends every thread of the run
        finally:
            a.close(), sink.close()
            fa.close()
        settle(start)
    gone.close()
    # a truncated input: the reader thread's ValueError, raised by get()
    run = streamio.Run()
    a, fa = source(run, data[:-3], 'lr', 2)
    try:
        a.header()
        a.provide(ring_of(fmt, 2))
        with pytest.raises(ValueError, match=r': truncated frame 5$'):
            while True:
                a.give(a.get()[1])
    finally:
        a.close()
        fa.close()
    settle(start)


# ------------------------------------------------------------------------------------------------ the options
def test_options(tmp_path):
    from refvsr_amd import videorun
    a, _ = file_bytes(tmp_path, 'i420', frames_of('i420', 2), name='a.y4m')
    b, _ = file_bytes(tmp_path, 'i420', frames_of('i420', 2), name='b.y4m')
    out = str(tmp_path / 'o.y4m')
    fifo = str(tmp_path / 'fifo.y4m')
    os.mkfifo(fifo)
    base = ['--lr', a, '--ref', b, '--out', out]
    cfg, _ = videorun.build_config(base)
    assert (cfg.EVAL.io, cfg.EVAL.io_depth, cfg.EVAL.io_timeout) == ('sync', 2, 120.0)
    cfg, _ = videorun.build_config(base + ['--io', 'stream', '--io_depth', '4', '--io_timeout', '7.5'])
    assert (cfg.EVAL.io, cfg.EVAL.io_depth, cfg.EVAL.io_timeout) == ('stream', 4, 7.5)
    # auto: stream as soon as one end is '-' or no regular file
    for argv in (['--lr', '-', '--ref', b, '--out', out], ['--lr', a, '--ref', '-', '--out', out], ['--lr', a, '--ref', b, '--out', '-'],
                 ['--lr', fifo, '--ref', b, '--out', out], ['--lr', a, '--ref', b, '--out', '/dev/null'], ['--lr', a, '--ref', fifo, '--out', out]):
        assert videorun.build_config(argv)[0].EVAL.io == 'stream', argv
        assert videorun.build_config(argv + ['--io', 'auto'])[0].EVAL.io == 'stream'
        with pytest.raises(ValueError, match=r'^videorun: --io sync reads and writes regular files \(.* is none\)'):
            videorun.build_config(argv + ['--io', 'sync'])
    assert videorun.build_config(base + ['--io', 'sync'])[0].EVAL.io == 'sync'
    for extra, text in ((['--io_depth', '0'], r'--io_depth must be an integer 1\.\.4 \(got 0\)'), (['--io_depth', '5'], r'--io_depth must be'),
                        (['--io_timeout', '0'], r'--io_timeout must be a positive number of seconds'), (['--io_timeout', 'nan'], r'--io_timeout must be')):
        with pytest.raises(ValueError, match=text) as e:
            videorun.build_config(base + extra)
        assert str(e.value).startswith('videorun: ') and '\n' not in str(e.value)
    for io_ in ('auto', 'stream', 'sync'):
        with pytest.raises(ValueError, match=r"^videorun: --lr and --ref cannot both be '-'"):
            videorun.build_config(['--lr', '-', '--ref', '-', '--out', out, '--io', io_])
    for extra in (['--io', 'async'], ['--io_depth', 'two']):
        with pytest.raises(SystemExit):
            videorun.build_config(base + extra)
    # the same checks behind run(): EVAL fields set by a caller
    assert videorun.io_mode(None, a, b, out) == 'sync' and videorun.io_mode('auto', a, io.BytesIO(), out) == 'stream'
    with pytest.raises(ValueError, match='--io must be one of sync, stream, auto'):
        videorun.io_mode('fast', a, b, out)
    assert videorun.check_io_depth(None) == 2 and videorun.check_io_timeout(None) == 120.0
    with pytest.raises(ValueError, match='--io_depth'):
        videorun.check_io_depth(2.5)
    assert videorun.held_bound(5, 4, 2) == 5 + 3 * 4 + 2
