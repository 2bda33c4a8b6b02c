"""The cases of tests/test_packing_golden.py and tests/test_conv_route.py: what is packed, what is called, how it is digested.

Every function takes the modules under test as arguments, so that the same case list ran against the packing.py / ops.py of the
commit before the weight path was restated (a scratch copy of those files, imported as a package) to record
tests/golden/packing_digests.json and tests/golden/conv_routes.json."""
import hashlib
import itertools

import numpy as np
import torch

CONFIGS = ('config_RefVSR_small_L1', 'config_RefVSR_small_MFID', 'config_RefVSR_L1', 'config_RefVSR_MFID', 'config_RefVSR_MFID_8K',
           'config_RefVSR_small_MFID_8K', 'config_RefVSR_IR_L1', 'config_RefVSR_IR_MFID')
FP16_CONFIGS = ('config_RefVSR_small_L1', 'config_RefVSR_small_MFID', 'config_RefVSR_small_MFID_8K')     # mid_channels = 24, RefVSR

# (cout, real source channels, pack_conv24 keywords): every (cout, pads) packing.conv24_ok accepts
CONV24_SHAPES = ([(24, s, {}) for s in ([24], [16], [3, 24], [24, 24])] + [(24, [48, 48], dict(half_group=True))] +
                 [(32, s, {}) for s in ([32], [3])] +
                 [(48, s, {}) for s in ([48], [16], [48, 48], [3, 48])] + [(48, [24], dict(shuffle_group=True))])


def weights(seed, cout, cin, fp16=False, ks=3):
    """(w [cout, cin, ks, ks], b [cout]) of about 0.1, so that the lo halves fp16(w - fp16(w)) are non-zero; fp16: rounded to fp16, what
    the engine hands the packers under weight_precision = 'fp16'."""
    rs = np.random.RandomState(seed)
    w, b = (0.1 * rs.standard_normal((cout, cin, ks, ks))).astype(np.float32), (0.1 * rs.standard_normal(cout)).astype(np.float32)
    if fp16:
        w, b = w.astype(np.float16).astype(np.float32), b.astype(np.float16).astype(np.float32)
    return torch.from_numpy(w), torch.from_numpy(b)


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p.encode() if isinstance(p, str) else p.contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def packer_digests(pk):
    """{case name: sha256 of the packed bytes} over the blob packers of the module pk."""
    out = {}
    for k, ((cout, srcs, kw), wfmt) in enumerate(itertools.product(CONV24_SHAPES, ('hi_lo', 'fp16'))):
        w, b = weights(100 + k, cout, sum(srcs), wfmt == 'fp16')
        out['pack_conv24 %d<-%s %s %s' % (cout, '+'.join(map(str, srcs)), ','.join(kw) or '-', wfmt)] = sha(pk.pack_conv24(w, b, srcs, wfmt=wfmt, **kw))
    for k, (c, wfmt) in enumerate(((24, 'hi_lo'), (24, 'fp16'), (48, 'hi_lo'))):
        w, b = weights(200 + k, 4 * c, c, wfmt == 'fp16')
        out['pack_conv_shuffle2 %d %s' % (c, wfmt)] = sha(pk.pack_conv_shuffle2(w, b, wfmt=wfmt))
    for k, (name, c, fp16) in enumerate((('pack_resblock24', 24, False), ('pack_resblock24_f16w', 24, True), ('pack_resblock48', 48, False))):
        (w1, b1), (w2, b2) = weights(300 + 2 * k, c, c, fp16), weights(301 + 2 * k, c, c, fp16)
        out[name] = sha(getattr(pk, name)(w1, b1, w2, b2))
    out['pack_conv_hr_last'] = sha(pk.pack_conv_hr_last(*weights(400, 24, 24), *weights(401, 3, 24)))
    for c in (24, 48):
        out['pack_conv_last %d' % c] = sha(pk.pack_conv_last(*weights(410 + c, 3, c)))
    return out


def model_cases():
    return [(c, None) for c in CONFIGS] + [(c, 'fp16') for c in FP16_CONFIGS]


_MODELS = {}


def model(refvsr_amd, engine, config, weight_precision=None, seed=1234):
    """(engine.Weights(config, make_state_dict(config, seed), 'cpu'), the distinct conv shapes it packed: sorted [(w_shape,
    src_channels, shuffle, f32, hi_only)]), built once per process."""
    key = (engine.__name__, engine.__file__, config, weight_precision, seed)
    if key not in _MODELS:
        cfg = refvsr_amd.get_config('p', 'm', config)
        if weight_precision:
            cfg.weight_precision = weight_precision
        shapes, real = set(), engine.pack_conv

        def spy(w, b, src_channels, shuffle=False, mt=None, f32=False, hi_only=False):
            shapes.add((tuple(w.shape), tuple(src_channels), bool(shuffle), bool(f32), bool(hi_only)))
            return real(w, b, src_channels, shuffle, mt=mt, f32=f32, hi_only=hi_only)
        engine.pack_conv = spy
        try:
            _MODELS[key] = (engine.Weights(cfg, refvsr_amd.make_state_dict(cfg, seed), 'cpu'), sorted(shapes))
        finally:
            engine.pack_conv = real
    return _MODELS[key]


def model_digest(refvsr_amd, engine, config, weight_precision=None):
    """sha256 over every conv of the model's packed weights, by name: wpack, bias, blob24 and blob_wfmt."""
    W, _ = model(refvsr_amd, engine, config, weight_precision)
    return sha(*[x for name, cw in sorted(W.conv.items()) for x in (name, cw.wpack, cw.bias, 'none' if cw.blob24 is None else cw.blob24, cw.blob_wfmt)])


# ---- the route of a conv call (tests/test_conv_route.py) ---------------------------------------------------------------------------
SUP24 = ((24, 0), (16, 0), (8, 24), (24, 24))     # refvsr_conv24_supported (tests/test_host.py pins packing.conv24_ok to the library's lists)
ACT_POST = tuple(itertools.product((0.0, 0.2, 1.5), (1.0, 0.2, 1.5)))
KNOBS = (None, 'REFVSR_NO_CONV24', 'REFVSR_NO_CONV32', 'REFVSR_NO_CONV48X2', 'REFVSR_NO_CONV_SHUFFLE2')


def conv_shapes(refvsr_amd, engine):
    """The distinct conv shapes of the eight configs."""
    return sorted(set(s for c in CONFIGS for s in model(refvsr_amd, engine, c)[1]))


def shape_name(shape):
    (cout, cin, ks, _), srcs, shuffle, f32, hi_only = shape
    return '%d<-%s k%d%s%s%s' % (cout, '+'.join(map(str, srcs)), ks, ' shuffle' if shuffle else '', ' f32' if f32 else '', ' hi_only' if hi_only else '')


def packed(pk, shape, k=0):
    (cout, cin, ks, _), srcs, shuffle, f32, hi_only = shape
    return pk.pack_conv(*weights(500 + k, cout, cin, ks=ks), list(srcs), shuffle, f32=f32, hi_only=hi_only)


def blob_code(has_blob, blob_wfmt):
    """'-': no specialised blob, 'h': one in the hi + lo format, 'f': one in the fp16 weight format."""
    return '-' if not has_blob else {'hi_lo': 'h', 'fp16': 'f'}[blob_wfmt]


def blob_table(ops, pk, shapes, set_knob):
    """{'<shape> | <wfmt>': blob_code for each of KNOBS, as one string} of ops.ConvWeights on the CPU; set_knob(name or None) switches
    one A/B knob on (None: all off) the way the ConvWeights under test reads it."""
    out = {}
    for k, shape in enumerate(shapes):
        p = packed(pk, shape, k)
        for wfmt in ('hi_lo', 'fp16'):
            codes = []
            for knob in KNOBS:
                set_knob(knob)
                cw = ops.ConvWeights(p, 'cpu', wfmt=wfmt)
                assert cw.blob24 is not None or cw.blob_wfmt == 'hi_lo'
                codes.append(blob_code(cw.blob24 is not None, cw.blob_wfmt))
            out['%s | %s' % (shape_name(shape), wfmt)] = ''.join(codes)
    set_knob(None)
    return out


class RecordingLib(object):
    """Stands in for the library: every entry point records its name and succeeds; refvsr_conv24_supported answers from SUP24."""

    def __init__(self):
        self.launches, self.queries = [], 0

    def __getattr__(self, name):
        if name == 'refvsr_conv24_supported':
            def query(c0, c1):
                self.queries += 1
                return int((c0, c1) in SUP24)
            return query

        def entry(*args):
            self.launches.append(name)
            return 0
        return entry


def _map(h, w, c, dtype, real):
    """An [h, w, c] map: real zeros, or one element viewed at that shape (stride 0: no memory behind the 2 GiB maps)."""
    return torch.zeros(h, w, c, dtype=dtype) if real else torch.zeros(1, dtype=dtype).expand(h, w, c)


def route_table(ops, hip, pk, shapes, setattr_):
    """{'<shape> | <wfmt> | <call> | <map> ': ['<first entry point> <launches> <queries>' or the exception's name, for each of
    ACT_POST]} of ops.conv / ops.conv_b on a RecordingLib.  Shapes: `shapes`, each as ops.ConvWeights on the CPU, in the fp16 weight
    format as well where that changes the blob.  Calls: conv plain (one source or two, as packed), with mul + res, planar_out +
    res_planar, stride 2; conv_b over B = 1 .. 5 maps plain and with muls + ress.  Maps: 4 x 6, and for every channel count M among
    (cout, c0, c1) the h x 4096 map at which h w M 2 bytes first reaches 2^31 (no planar form on those).
    setattr_(object, name, value): monkeypatch.setattr."""
    lib = RecordingLib()
    setattr_(hip, 'lib', lambda: lib)
    setattr_(ops, '_stream', lambda: None)
    setattr_(ops, '_nhwc', lambda t, f32=False: t)
    setattr_(ops, '_planar', lambda t, c=None: t)
    empty = torch.empty
    setattr_(torch, 'empty', lambda shape, dtype=None, device=None: empty(1, dtype=dtype).expand(tuple(shape)))
    out = {}
    for k, shape in enumerate(shapes):
        p = packed(pk, shape, k)
        cout = shape[0][0]
        for wfmt in ('hi_lo', 'fp16'):
            cw = ops.ConvWeights(p, 'cpu', wfmt=wfmt)
            if wfmt == 'fp16' and cw.blob_wfmt != 'fp16':
                continue
            if len(cw.cpads) == 3:                  # RefVSR_IR's three-source conv: engine.Weights hands the first two over as one map
                cw.cpads = [cw.cpads[0] + cw.cpads[1], cw.cpads[2]]
            dt = torch.float32 if cw.f32 else torch.float16
            co = cout // 4 if cw.shuffle else cout                     # channels of the output map (what mul / res have)
            maps = [('4x6', 4, 6)] + [('2^31/%d' % m, -(-2 ** 18 // m), 4096) for m in sorted(set([cout] + list(cw.cpads)))]
            for mname, h, w in maps:
                real = mname == '4x6'
                srcs = [_map(h, w, c, dt, real) for c in cw.cpads]
                mr = dict(mul=_map(h, w, co, dt, real), res=_map(h, w, co, dt, real))
                calls = [('conv', lambda a, q: ops.conv(cw, *srcs, act=a, post=q)),
                         ('conv mul+res', lambda a, q: ops.conv(cw, *srcs, act=a, post=q, **mr)),
                         ('conv stride2', lambda a, q: ops.conv(cw, *srcs, stride=2, act=a, post=q))]
                if real:
                    rp = torch.zeros(cout, h, w)
                    calls.append(('conv planar', lambda a, q: ops.conv(cw, *srcs, act=a, post=q, planar_out=True, res_planar=rp)))
                for B in range(1, 6):
                    ls = [[s] * B for s in srcs]
                    calls.append(('conv_b B=%d' % B, lambda a, q, ls=ls: ops.conv_b(cw, *ls, act=a, post=q, stack=False)))
                    calls.append(('conv_b B=%d muls+ress' % B, lambda a, q, ls=ls, B=B: ops.conv_b(
                        cw, ls[0], ls[1] if len(ls) > 1 else None, act=a, muls=[mr['mul']] * B, ress=[mr['res']] * B, post=q, stack=False)))
                for cname, call in calls:
                    row = []
                    for a, q in ACT_POST:
                        del lib.launches[:]
                        lib.queries = 0
                        try:
                            call(a, q)
                            row.append('%s %d %d' % (lib.launches[0], len(lib.launches), lib.queries))
                        except Exception as e:      # (a call the wrappers refuse: the refusal is the recorded outcome)
                            row.append(type(e).__name__)
                    out['%s | %s | %s | %s' % (shape_name(shape), wfmt, cname, mname)] = row
    return out


def pack_table(table):
    """A route table in the form of the golden file: {'outcomes': the distinct outcome strings, 'patterns': the distinct rows as
    outcome numbers, 'rows': {'<shape> | <wfmt>': the pattern number of each of its rows, in the table's order}}."""
    outcomes = sorted(set(o for row in table.values() for o in row))
    rows = {k: [outcomes.index(o) for o in row] for k, row in table.items()}
    patterns = sorted(set(map(tuple, rows.values())))
    out = {}
    for k, row in rows.items():
        out.setdefault(' | '.join(k.split(' | ')[:2]), []).append(patterns.index(tuple(row)))
    return dict(outcomes=outcomes, patterns=[list(p) for p in patterns], rows=out)


def unpack_table(packed_, keys):
    """The table pack_table() made, under the row names `keys` (a table of the same cases, in its order)."""
    pos, out = {}, {}
    for k in keys:
        group = ' | '.join(k.split(' | ')[:2])
        i = pos[group] = pos.get(group, -1) + 1
        out[k] = [packed_['outcomes'][o] for o in packed_['patterns'][packed_['rows'][group][i]]]
    assert {g: n + 1 for g, n in pos.items()} == {g: len(r) for g, r in packed_['rows'].items()}
    return out
