"""The input source: the ONE description of what a window's frames are made of.  source_of() answers with one of three small objects --
float32 RGB frames, uint8 RGB frames (value = byte / 255), Y'CbCr 4:2:0 frames [3h/2, w] (config.input_yuv) -- that answer the same
questions; the engine's contexts, window cache and checks and the network's entry check ask them instead of telling the kinds apart.
Every device entry point is reached through the `ops` module attribute at call time, so a test that replaces one replaces it here too."""
import torch

from . import ops, yuv


class _Float(object):
    """float32 RGB frames [3,h,w]: a context's frames are its clones of the caller's, compared as they are."""
    key = None                  # the hashable that decides whether two contexts may match by content (FrameCtx.kind)
    keeps_source = False        # whether a context keeps its copies of the source samples (FrameCtx.src) beside its fp32 frames

    def geometry(self, x):
        """(h, w) of a frame or window of this kind."""
        return tuple(x.shape[-2:])

    def frames(self, copies):
        """(the fp32 frames (lr, ref) of a context that made `copies` of its source frames, the (source, frame) pairs still to decode)."""
        if not self.keeps_source:
            return copies, []
        out = tuple(torch.empty((3,) + tuple(self.geometry(c)), dtype=torch.float32, device=c.device) for c in copies)
        return out, list(zip(copies, out))

    def decode(self, pairs):
        """Fill the fp32 frames of [(source copy, frame)], one launch per 16 frames (a call collects the pairs of its new contexts)."""
        assert not pairs, 'the windows of one call are of one kind'

    def equal(self, pairs):
        """[bool] per pair (a caller's frame, what a context holds of it: own(ctx)[0 | 1]); one launch per 32 pairs, one D2H sync."""
        return ops.buffers_equal(pairs)

    def own(self, ctx):
        return ctx.lr, ctx.ref


class _Bytes(_Float):
    """uint8 RGB frames: the byte copies (a quarter of the fp32 size, in the caller's layouts) key the content compare, the fp32 frames
    are filled by refvsr_ingest_u8.  key: the layouts (ops.u8_layout) of lr and ref, None for strides the kernel does not read."""
    keeps_source = True

    def __init__(self, lrs, refs):
        self._of = (lrs, refs)

    @property
    def key(self):
        return ops.u8_layout(self._of[0]), ops.u8_layout(self._of[1])

    def decode(self, pairs):
        ops.ingest_u8(pairs)

    def equal(self, pairs):
        return ops.bytes_equal(pairs)

    def own(self, ctx):
        return ctx.src


class _Yuv420(_Bytes):
    """4:2:0 frames [3h/2, w] under config.input_yuv resolved (format, matrix, range, chroma): the copies of the source samples (half
    the bytes of the uint8 kind) key the compare, the fp32 frames are filled by refvsr_yuv420_to_rgb.  Also the 4:2:2 / 4:4:4 formats
    ([2h, w] / [3h, w] frames) and left-sited chroma (a fifth parameter, yuv.resolve_input): those go through refvsr_yuv_to_rgb (ops.yuv_decode
    chooses).  The format -- and so the sampling -- and the siting are part of the key: the same bytes under another declaration never
    match."""

    def __init__(self, params):
        self.params = tuple(params)

    @property
    def key(self):
        return ('yuv',) + self.params

    def geometry(self, x):
        return ops.yuv_geometry(x) if self.params[0] in yuv.FORMATS else ops.yuv_geometry(x, self.params[0])

    def decode(self, pairs):
        if pairs:
            ops.yuv_decode(pairs, self.params)


_FLOAT = _Float()


def source_of(lrs, refs, input_yuv=None):
    """The source of the frames or windows lrs, refs under Engine.input_yuv (None, or config.input_yuv resolved).  Contexts of another
    key never match by content: a float frame is not compared with a byte frame, nor a planar ref with a channels-last one."""
    if input_yuv is not None:
        return _Yuv420(input_yuv)
    return _FLOAT if lrs.dtype != torch.uint8 else _Bytes(lrs, refs)


def as_is(x):
    """True for an RGB tensor that is read without a conversion: contiguous float32, or uint8 contiguous / channels-last."""
    return ops.u8_layout(x) is not None if x.dtype == torch.uint8 else x.dtype == torch.float32 and x.is_contiguous()


def check_window(lrs, refs, fmt, dim, what, lead):
    """lrs, refs are a window of `dim` dimensions [<lead>, 3, h, w] for this configuration -- under config.input_yuv = fmt of dim - 1
    dimensions [<lead>, 3h/2, w]: dense cuda 4:2:0 frames of the format's sample type and of one shape; otherwise RGB, both bytes or
    both float (what else an entry asks of RGB windows, convert or refuse, is its own).  RuntimeError, one line, otherwise."""
    if fmt is not None:
        dt = torch.uint8 if yuv.depth_of(fmt) == 8 else torch.uint16
        rows = {'420': '3h/2', '422': '2h', '444': '3h'}[yuv.sampling_of(fmt)]
        for x in (lrs, refs):
            if not (x.is_cuda and x.dim() == dim - 1 and x.dtype == dt and x.shape == lrs.shape and ops.yuv_window_kind(x, fmt) is not None):
                raise RuntimeError("input_yuv = '%s': lrs and refs must be contiguous cuda %s [%s, %s, w] windows of one shape, %s rows with even "
                                   "h and w (got %s %s%s)" % (fmt, dt, lead, rows, rows, x.dtype, tuple(x.shape), '' if x.is_contiguous() else ', not contiguous'))
    elif lrs.dim() == dim - 1:
        raise RuntimeError("%s: windows are float or uint8 [.., t, 3, h, w]; [.., t, 3h/2, w] Y'CbCr 4:2:0 windows need config.input_yuv "
                           "(got %s %s)" % (what, lrs.dtype, tuple(lrs.shape)))
    elif (lrs.dtype == torch.uint8) != (refs.dtype == torch.uint8):
        raise RuntimeError('%s: lrs and refs must both be uint8 or both float (got %s and %s)' % (what, lrs.dtype, refs.dtype))
