#!/usr/bin/env python3
"""Generate golden fixtures by running the REAL reference (/root/reference) on CPU.

Runs only in the build container (the reference does not travel to the GPU box).  The reference
is imported unmodified; four un-vendored third-party packages it imports (mmcv, torchvision,
termcolor, easydict -- absent from this image, no network) are replaced by the minimal stand-ins
in tools/ref_shims/ (SURVEY.md section 8c / appendix B).  Nothing from the reference is copied:
only input/output tensors are written to tests/golden/*.npz.

    python tools/gen_golden.py            # writes tests/golden/*.npz and prints oracle deltas
    python tools/gen_golden.py --plugin-spec   # only tests/golden/plugin_state_dict.json (the reference shell's state dict)
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, '/root/reference')

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from refvsr_amd import weights as wts  # noqa: E402
from refvsr_amd.config import get_config as my_get_config  # noqa: E402
from oracle import refvsr_oracle as orc  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
VIS_FIXTURES = ('S_18x26_t5', 'HD_32x48_t3')
SEED_W = 1234


def ref_net(name, frame_num, save_sample=True, scale=4):
    cfg = importlib.import_module('configs.' + name).get_config('p', 'm', name)
    if scale != 4:            # what editing `config.scale = 4 # SR scale (2 | 4)` in the reference's config file does (:30-39)
        cfg.scale = scale
        cfg.matching_ksize = (4 if scale == 2 else 2) * (scale if cfg.flag_HD_in else 1)
    cfg.cuda = False
    cfg.device = 'cpu'
    cfg.dist = False
    cfg.frame_num = frame_num
    cfg.save_sample = save_sample
    from models.SRNet import SRNet
    net = SRNet(cfg).eval()
    mine = my_get_config('p', 'm', name)
    mine.frame_num = frame_num
    mine.save_sample = save_sample
    if scale != 4:
        from refvsr_amd.config import set_scale
        set_scale(mine, scale)
    # the build's config mirror must agree with the reference on every model field
    for k in ('scale', 'flag_HD_in', 'matching_ksize', 'num_blocks', 'mid_channels', 'reset_branch',
              'is_amp', 'network') + (('keyframe_stride',) if 'IR' in name else ()):
        assert cfg[k] == mine[k], (name, k, cfg[k], mine[k])
    sd = wts.make_state_dict(mine, SEED_W)
    ref_sd = net.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()) or set(ref_sd.keys()) == set(sd.keys()), \
        set(ref_sd.keys()) ^ set(sd.keys())
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(sd[k].shape), (k, v.shape, sd[k].shape)
    net.load_state_dict(sd, strict=True)
    return net, cfg, mine, sd


def rnd(rs, *shape):
    return torch.from_numpy(rs.rand(*shape).astype(np.float32))


def quant8(x):
    return torch.round(x * 255.0) / 255.0          # data_loader/utils.py:20,28 (8-bit frames)


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = v
    path = os.path.join(GOLD, name + '.npz')
    np.savez_compressed(path, **out)
    print('  wrote %-34s %7.1f KB' % (name + '.npz', os.path.getsize(path) / 1024.0))


def md(a, b):
    return float((a - b).abs().max())


def gen_ops():
    """Per-op goldens on the small (S) weights."""
    print('== per-op goldens (RefVSR_small_L1 weights) ==')
    net, cfg, mine, sd = ref_net('config_RefVSR_small_L1', 5)
    N = net.Network
    rs = np.random.RandomState(7)
    from models.utils import warp as ref_warp
    from mmedit.models.common import flow_warp as ref_flow_warp
    from models.archs.RefVSR_.utils import extract_image_patches
    with torch.no_grad():
        # warp (LR form and LR-input / 2x-flow form)
        x = rnd(rs, 1, 5, 18, 26)
        fl = (rnd(rs, 1, 2, 18, 26) - 0.5) * 6
        fl2 = (rnd(rs, 1, 2, 36, 52) - 0.5) * 10
        w1, w2 = ref_warp(x, fl), ref_warp(x, fl2)
        print('  warp          ', md(w1, orc.warp(x, fl)), md(w2, orc.warp(x, fl2)))
        fw = ref_flow_warp(x, fl.permute(0, 2, 3, 1), padding_mode='border')
        print('  flow_warp     ', md(fw, orc.flow_warp_border(x, fl)))
        save('op_warp', x=x, flow=fl, flow2=fl2, warp=w1, warp2=w2, flow_warp=fw)
        # resizes
        img = rnd(rs, 1, 3, 18, 26)
        b05 = F.interpolate(img, scale_factor=0.5, mode='bicubic', align_corners=False)
        b2 = F.interpolate(img, scale_factor=2, mode='bicubic', align_corners=False)
        b4 = F.interpolate(img, scale_factor=4, mode='bicubic', align_corners=False)
        up = F.interpolate(fl, scale_factor=2, mode='bilinear', align_corners=True) * 2.0
        bl = F.interpolate(img, size=(32, 32), mode='bilinear', align_corners=False)
        bl_back = F.interpolate(bl, size=(18, 26), mode='bilinear', align_corners=False)
        nn_ = F.interpolate(img, scale_factor=0.5, mode='nearest')
        print('  bicubic       ', md(b05, orc.bicubic_scale(img, 0.5, False)), md(b2, orc.bicubic_scale(img, 2, False)),
              md(b4, orc.bicubic_scale(img, 4, False)))
        print('  bilinear      ', md(up, orc.flow_up2(fl)), md(bl, orc.resize(img, (32, 32), 'bilinear')),
              md(bl_back, orc.resize(bl, (18, 26), 'bilinear')), md(nn_, orc.resize(img, (9, 13), 'nearest', 2.0)))
        save('op_resize', img=img, flow=fl, bicubic_half=b05, bicubic_x2=b2, bicubic_x4=b4, flow_up2=up,
             bilinear_32x32=bl, bilinear_back=bl_back, nearest_half=nn_)
        # patch extraction
        f16 = rnd(rs, 1, 4, 10, 12)
        pt = extract_image_patches(f16, [3, 3], [1, 1], [1, 1], 'same')
        print('  patches3x3    ', md(pt, orc.patches3x3(f16)))
        save('op_patches', f=f16, patches=pt)
        # feature matching
        lr = quant8(rnd(rs, 1, 3, 20, 28))
        rf = quant8(rnd(rs, 1, 3, 20, 28))
        conf, idx = N.feature_match(lr, rf)
        oc, oi = orc.feature_match(lr, rf, sd, False)
        print('  feature_match ', md(conf, oc), int((idx != oi).sum()), 'idx mismatches')
        save('op_match', lr=lr, ref=rf, conf=conf, idx=idx)
        # block gathers (aa1: s=1 from LR/2 features; aa2: s=2 from LR features)
        C = mine.mid_channels
        vd = rnd(rs, 1, C, 10, 14)
        v = rnd(rs, 1, C, 20, 28)
        lr_down = F.interpolate(lr, scale_factor=0.5, mode='bicubic', align_corners=False)
        g1 = N.aa1(lr_down, rf, idx, vd, 'aa1')
        g2 = N.aa2(lr, rf, idx, v, 'aa2', return_fm=True)
        g2rgb = N.aa2(lr, rf, idx, rf, 'aa2', return_fm=True)
        print('  block_gather  ', md(g1, orc.block_gather(vd, idx, 1, (20, 28))),
              md(g2, orc.block_gather(v, idx, 2, (40, 56))), md(g2rgb, orc.block_gather(rf, idx, 2, (40, 56))))
        # full aa2 incl. AlignedConv2d
        a2 = N.aa2(lr, rf, idx, v, 'aa2')
        oa2 = orc.aligned_conv(orc.block_gather(v, idx, 2, (40, 56)), lr, orc.block_gather(rf, idx, 2, (40, 56)),
                               sd, 'Network.aa2.align', 2)
        print('  aa2+align     ', md(a2, oa2))
        save('op_aa', lr=lr, ref=rf, idx=idx, value_down=vd, value=v, aa1=g1, aa2_fm=g2, aa2_rgb=g2rgb, aa2=a2)
        # sampler alone with a hand-made affine field (exercises clamping, rotation, scaling)
        xs = rnd(rs, 1, 3, 12, 16)
        aff = torch.stack([rnd(rs, 6, 8) * 4 - 1, rnd(rs, 6, 8) * 4 - 1, rnd(rs, 6, 8) * 6 - 3])[None]
        A = N.aa2.align
        # drive the reference's own AlignedConv2d.forward with an injected affine field: its encoder is
        # bypassed (identity) and its predictor replaced by a constant, so only the sampler runs.
        class _Const(torch.nn.Module):
            def forward(self, z):
                return aff - 1.0
        keep = (A.p_conv, A.conv1)
        A.p_conv, A.conv1 = _Const(), torch.nn.Identity()
        smp = A(xs, torch.zeros(1, 3, 6, 8), torch.zeros(1, 3, 12, 16))
        A.p_conv, A.conv1 = keep
        print('  aligned_sample', md(smp, orc.aligned_sample(xs, aff.clamp(-3, 3), 2)))
        save('op_sampler', x=xs, affine=aff.clamp(-3, 3), out=smp)
        # SPyNet (non-/32 size)
        a = quant8(rnd(rs, 1, 3, 36, 52))
        sh = torch.roll(a, shifts=(1, 2), dims=(2, 3))
        flo = N.FlowNet(a, sh)
        print('  spynet        ', md(flo, orc.spynet(a, sh, sd)))
        save('op_spynet', a=a, b=sh, flow=flo)
        # conv stacks
        ft = rnd(rs, 1, C, 12, 16) - 0.5
        rl = N.feat_decoder2(ft)
        rb = N.backward_resblocks(torch.cat([a[:, :, :12, :16], ft], 1))
        ps = N.upsample1(ft)
        print('  reslist/resblocks/pixelshuffle', md(rl, orc.res_list(ft, sd, 'Network.feat_decoder2', 4)),
              md(rb, orc.resblocks_with_input_conv(torch.cat([a[:, :, :12, :16], ft], 1), sd, 'Network.backward_resblocks', mine.num_blocks)),
              md(ps, orc.pixel_shuffle_pack(ft, sd, 'Network.upsample1')))
        save('op_convs', feat=ft, img=a[:, :, :12, :16], res_list=rl, resblocks=rb, pixel_shuffle=ps)
        # upsampler
        bw = rnd(rs, 1, C, 12, 16) - 0.5
        fwd = rnd(rs, 1, C, 12, 16) - 0.5
        cb, cf = rnd(rs, 1, 1, 6, 8), rnd(rs, 1, 1, 6, 8)
        base = rnd(rs, 1, 3, 24, 32)
        cu = N.compute_up(bw, fwd, cb, cf, base)
        o = orc.OracleNetwork(mine, sd)
        print('  compute_up    ', md(cu, o._compute_up(bw, fwd, cb, cf, base)))
        save('op_compute_up', bw=bw, fw=fwd, conf_bw=cb, conf_fw=cf, base=base, out=cu)


def synth_clip(rs, nframes, h, w):
    """Smooth moving texture so flows / matches are non-trivial; 8-bit quantised like read_frame."""
    H, W = h + 8, w + 8 + nframes
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((3, H, W), np.float32)
    for c in range(3):
        for _ in range(6):
            fy, fx, ph = rs.uniform(0.05, 0.9), rs.uniform(0.05, 0.9), rs.uniform(0, 6.28)
            img[c] += rs.uniform(0.3, 1.0) * np.sin(fy * yy + fx * xx + ph)
    img = (img - img.min()) / (img.max() - img.min()) * 0.9 + 0.05
    img += rs.uniform(-0.03, 0.03, img.shape).astype(np.float32)
    lrs, refs = [], []
    for f in range(nframes):
        lrs.append(img[:, 4:4 + h, f:f + w])
        refs.append(img[:, 2:2 + h, f + 3:f + 3 + w][:, ::1, ::1])
    lr = torch.from_numpy(np.stack(lrs)[None].copy()).clamp(0, 1)
    rf = torch.from_numpy(np.stack(refs)[None].copy()).clamp(0, 1)
    return quant8(lr), quant8(rf)


def windows(nframes, t):
    """Sliding windows with edge-frame repetition (data_loader/datasets.py:222-234)."""
    out = []
    for f in range(nframes):
        out.append([min(max(f - t // 2 + k, 0), nframes - 1) for k in range(t)])
    return out


def gen_e2e(tag, name, t, h, w, nframes, reset_override='keep', light=False, scale=4):
    print('== end-to-end %s: %s t=%d %dx%d, %d frames, x%d ==' % (tag, name, t, h, w, nframes, scale))
    net, cfg, mine, sd = ref_net(name, t, scale=scale)
    if reset_override != 'keep':
        cfg.reset_branch = reset_override
        mine.reset_branch = reset_override
        net.Network.max_frame_itr_num = reset_override
    rs = np.random.RandomState(abs(hash(tag)) % (2 ** 31) if False else sum(map(ord, tag)))
    lr, rf = synth_clip(rs, nframes, h, w)
    o = orc.OracleNetwork(mine, sd)
    arrs = dict(lr=lr, ref=rf, t=np.int64(t), reset_branch=np.int64(-1 if mine.reset_branch is None else mine.reset_branch),
                scale=np.int64(scale))
    with torch.no_grad():
        for f, win in enumerate(windows(nframes, t)):
            x, r = lr[:, win], rf[:, win]
            first = (f == 0)
            outs = net(x, r, first, is_log=True, is_train=False)
            tr = {}
            oo = o.forward(x, r, first, is_log=True, trace=tr)
            N = net.Network
            d = dict(result=md(outs['result'], oo['result']),
                     feat=md(N.forward_feat_prop_prev, o.forward_feat_prop_prev),
                     feat_up=md(N.forward_feat_prop_UP_prev, o.forward_feat_prop_UP_prev),
                     conf=md(N.forward_conf_map_prop_prev, o.forward_conf_map_prop_prev),
                     flow=md(N.forward_flow_prev, o.forward_flow_prev))
            res = outs['result']
            sat = float(((res <= 0) | (res >= 1)).float().mean())
            print('  frame %d first=%s itr=%d  ' % (f, tr['is_first_frame'], N.frame_itr_num) +
                  ' '.join('%s=%.2e' % kv for kv in d.items()) +
                  '  | result mean %.3f std %.3f sat %.3f |feat| %.2f |feat_up| %.2f' % (
                      float(res.mean()), float(res.std()), sat, float(N.forward_feat_prop_prev.abs().mean()),
                      float(N.forward_feat_prop_UP_prev.abs().mean())))
            assert N.frame_itr_num == o.frame_itr_num
            arrs['result_%d' % f] = outs['result']
            arrs['state_feat_%d' % f] = N.forward_feat_prop_prev.to(torch.float16) if light else N.forward_feat_prop_prev
            if not light:             # (light fixtures of the big models: the 2x state map alone is 2.4 MB per frame)
                arrs['state_feat_up_%d' % f] = N.forward_feat_prop_UP_prev.to(torch.float16) if h * w > 600 else N.forward_feat_prop_UP_prev
            arrs['state_conf_%d' % f] = N.forward_conf_map_prop_prev
            arrs['state_flow_%d' % f] = N.forward_flow_prev
            arrs['itr_%d' % f] = np.int64(N.frame_itr_num)
            for k, v in outs['eval_vis'].items():
                arrs['ev_%s_%d' % (k, f)] = v
            # the `vis` debugging samples (RefVSR.py:219-221,262-263,301-316): oracle delta for every stream, values stored
            # for the streams listed in VIS_FIXTURES (the maps are 2x-size RGB, they would double the other fixtures)
            dv = {k: md(v, oo['vis'][k]) for k, v in outs['vis'].items()}
            assert set(outs['vis']) == set(oo['vis']), (sorted(outs['vis']), sorted(oo['vis']))
            print('    vis: ' + ' '.join('%s=%.1e' % kv for kv in dv.items()))
            if tag in VIS_FIXTURES:
                for k, v in outs['vis'].items():
                    arrs['vis_%s_%d' % (k, f)] = v
    save('e2e_' + tag, **arrs)


def gen_e2e_ir(tag, name, t, h, w, nframes, reset_override='keep'):
    """RefVSR_IR (EDVR-M information refill, modulated deformable convs through tools/ref_shims/mmcv/ops): result, carried
    state, iteration counter and key-frame indices per call."""
    from oracle import refvsr_ir_oracle as iro
    print('== end-to-end %s: %s t=%d %dx%d, %d frames ==' % (tag, name, t, h, w, nframes))
    net, cfg, mine, sd = ref_net(name, t)
    if reset_override != 'keep':
        cfg.reset_branch = mine.reset_branch = reset_override
        net.Network.max_frame_itr_num = reset_override
    rs = np.random.RandomState(sum(map(ord, tag)))
    lr, rf = synth_clip(rs, nframes, h, w)
    o = iro.OracleNetworkIR(mine, sd)
    arrs = dict(lr=lr, ref=rf, t=np.int64(t), reset_branch=np.int64(-1 if mine.reset_branch is None else mine.reset_branch))
    with torch.no_grad():
        for f, win in enumerate(windows(nframes, t)):
            x, r = lr[:, win], rf[:, win]
            outs = net(x, r, f == 0, is_log=True, is_train=False)          # is_log: the `vis` samples (RefVSR_IR.py:367-384)
            oo = o.forward(x, r, f == 0, is_log=True)
            assert list(outs['vis'].keys()) == list(oo['vis'].keys()), (list(outs['vis'].keys()), list(oo['vis'].keys()))
            if f < 2:                                                       # (the later calls repeat the first two after the reset)
                for k, v in outs['vis'].items():
                    arrs['vis_%s_%d' % (k, f)] = v
            print('  vis: ' + ' '.join('%s=%.2e' % (k, md(v, oo['vis'][k])) for k, v in outs['vis'].items()))
            N = net.Network
            d = dict(result=md(outs['result'], oo['result']), feat=md(N.forward_feat_prop_prev, o.forward_feat_prop_prev),
                     feat_up=md(N.forward_feat_prop_UP_prev, o.forward_feat_prop_UP_prev),
                     conf=md(N.forward_conf_map_prop_prev, o.forward_conf_map_prop_prev), flow=md(N.forward_flow_prev, o.forward_flow_prev))
            res = outs['result']
            print('  frame %d itr=%d keyframes=%s  ' % (f, N.frame_itr_num, list(N.keyframe_idx)) + ' '.join('%s=%.2e' % kv for kv in d.items()) +
                  '  | result mean %.3f std %.3f sat %.3f' % (float(res.mean()), float(res.std()), float(((res <= 0) | (res >= 1)).float().mean())))
            assert N.frame_itr_num == o.frame_itr_num and list(N.keyframe_idx) == list(o.keyframe_idx)
            arrs['result_%d' % f] = res
            arrs['state_feat_%d' % f] = N.forward_feat_prop_prev.to(torch.float16)
            arrs['state_conf_%d' % f] = N.forward_conf_map_prop_prev
            arrs['state_flow_%d' % f] = N.forward_flow_prev
            arrs['itr_%d' % f] = np.int64(N.frame_itr_num)
            arrs['keyframes_%d' % f] = np.asarray(N.keyframe_idx, np.int64)
    save('e2e_' + tag, **arrs)


def gen_full(nframes=2, stride=8):
    """Full BASELINE size (270x480 -> 1080x1920, t=5), random AND 'plausible' weights: PSNR scalars, a strided
    sub-sample of the result, two full-resolution 128x128 crops per frame (the full frame is 24.9 MB) and -- the
    matching is where fp16 near-ties would show -- the index map and confidence map of every window's centre frame
    (they depend on the frame and the VGG head only, so they are stored once).  ~3 min + 1.5 min per frame and
    variant on 8 cores, 18 GB RSS."""
    from refvsr_amd.synth import make_clip, window_indices
    import time
    lr, rf, gt = make_clip(nframes, 270, 480, seed=0)
    crops = [(300, 500), (700, 1400)]                 # top-left corners of the 128x128 full-resolution crops
    arrs = dict(nframes=np.int64(nframes), stride=np.int64(stride), crops=np.asarray(crops, np.int64),
                lr_checksum=np.float64(lr.double().sum().item()), ref_checksum=np.float64(rf.double().sum().item()))
    variants = (None, 'plausible')
    if '--variant' in sys.argv:                       # regenerate one variant, keep the other from the existing file
        variants = (sys.argv[sys.argv.index('--variant') + 1],)
        variants = (None,) if variants[0] == 'random' else variants
        old = np.load(os.path.join(GOLD, 'e2e_full_S_270x480_t5.npz'))
        keep = (lambda k: k.startswith('p_')) if variants[0] is None else (lambda k: not k.startswith('p_'))
        for k in old.files:
            if keep(k):
                arrs[k] = old[k]
    for variant in variants:
        tag = '' if variant is None else 'p_'
        print('== full-size S 270x480 t=5, %d frames, weights: %s ==' % (nframes, variant or 'random'))
        net, cfg, mine, sd = ref_net('config_RefVSR_small_L1', 5, save_sample=False)
        if variant:
            net.load_state_dict(wts.make_state_dict(mine, SEED_W, variant=variant), strict=True)
        matches = []
        hook = net.Network.feature_match.register_forward_hook(lambda m, i, o: matches.append((o[0].clone(), o[1].clone())))
        with torch.no_grad():
            for f in range(nframes):
                w = window_indices(f, nframes, 5)
                del matches[:]
                t0 = time.time()
                res = net(lr[w][None], rf[w][None], f == 0, is_log=False, is_train=False)['result']
                mse = torch.mean((res - gt[f][None]) ** 2)
                p = float(10 * torch.log10(1 / mse))
                print('  frame %d: %.1f s, PSNR vs GT %.6f dB' % (f, time.time() - t0, p))
                arrs[tag + 'psnr_%d' % f] = np.float64(p)
                for ci, (y0, x0) in enumerate(crops):
                    arrs[tag + 'crop%d_%d' % (ci, f)] = res[0, :, y0:y0 + 128, x0:x0 + 128].clone()
                if variant is None:
                    arrs['sub_%d' % f] = res[0, :, ::stride, ::stride].clone()
                    # feature_match is called for window positions range_start..t-1: the centre frame is call ctr - range_start
                    conf, idx = matches[2 if f == 0 else 0]
                    arrs['conf_%d' % f] = conf[0, 0].clone()
                    arrs['idx_%d' % f] = idx[0].to(torch.int32).clone()
        hook.remove()
    save('e2e_full_S_270x480_t5', **arrs)


def gen_full_mfid(nframes=2, stride=8):
    """Full BASELINE size (270x480 -> 1080x1920, t=5) for BASELINE configs[2]'s model (config_RefVSR_MFID: C = 48, 30 blocks),
    random weights: PSNR scalars, the strided sub-sample and the two 128x128 full-resolution crops per frame (the matching does
    not depend on the model width: its index / confidence maps are pinned by the S fixture).  ~8 min per frame on 8 cores."""
    from refvsr_amd.synth import make_clip, window_indices
    import time
    lr, rf, gt = make_clip(nframes, 270, 480, seed=0)
    crops = [(300, 500), (700, 1400)]
    arrs = dict(nframes=np.int64(nframes), stride=np.int64(stride), crops=np.asarray(crops, np.int64),
                lr_checksum=np.float64(lr.double().sum().item()), ref_checksum=np.float64(rf.double().sum().item()))
    print('== full-size F (config_RefVSR_MFID) 270x480 t=5, %d frames, random weights ==' % nframes)
    net, cfg, mine, sd = ref_net('config_RefVSR_MFID', 5, save_sample=False)
    with torch.no_grad():
        for f in range(nframes):
            w = window_indices(f, nframes, 5)
            t0 = time.time()
            res = net(lr[w][None], rf[w][None], f == 0, is_log=False, is_train=False)['result']
            p = float(10 * torch.log10(1 / torch.mean((res - gt[f][None]) ** 2)))
            print('  frame %d: %.1f s, PSNR vs GT %.6f dB' % (f, time.time() - t0, p), flush=True)
            arrs['psnr_%d' % f] = np.float64(p)
            for ci, (y0, x0) in enumerate(crops):
                arrs['crop%d_%d' % (ci, f)] = res[0, :, y0:y0 + 128, x0:x0 + 128].clone()
            arrs['sub_%d' % f] = res[0, :, ::stride, ::stride].clone()
    save('e2e_full_F_270x480_t5', **arrs)


def gen_full_hd(h=1080, w=1920, nframes=2, stride=32, t=3):
    """BASELINE configs[4] at its stated size: config_RefVSR_MFID_8K (C = 48, 30 blocks, flag_HD_in: matching on nearest x0.5 +
    VGG19[0:7] features, aa1 scale 4 + align, aa2 scale 8 + align; configs/config_RefVSR_MFID_8K.py, RefVSR_/attention.py:65-67,93-98,
    RefVSR.py:39-40) on a 1080 x 1920 -> 4320 x 7680 synthetic clip, t = 3 (frame_num is a CLI value), random weights: one first-frame
    call + one steady call.  Stored: PSNR scalars vs the synthetic GT, two 128 x 128 crops at output resolution, a strided sub-sample
    of the result, and the centre frame's index map + (strided) confidence map.  The 8K result is 398 MB per frame -- never stored.
    Takes about 1 h on 8 cores and 40-50 GB of RSS (the reference materialises the 32 400 x 129 600 fp32 score matrix and several
    48-channel 8K maps)."""
    from refvsr_amd.synth import make_clip, window_indices
    import time
    tag = 'e2e_full_HD_%dx%d_t%d' % (h, w, t)
    clip_n = nframes + t // 2
    lr, rf, gt = make_clip(clip_n, h, w, seed=0)
    gt = gt[:nframes].clone()
    s = 4
    crops = [(int(1.1 * h), int(1.05 * w)), (int(2.6 * h), int(2.9 * w))]
    arrs = dict(nframes=np.int64(nframes), clip_frames=np.int64(clip_n), stride=np.int64(stride), crops=np.asarray(crops, np.int64),
                t=np.int64(t), h=np.int64(h), w=np.int64(w),
                lr_checksum=np.float64(lr.double().sum().item()), ref_checksum=np.float64(rf.double().sum().item()))
    print('== full-size HD (config_RefVSR_MFID_8K) %dx%d t=%d, %d frames, random weights ==' % (h, w, t, nframes), flush=True)
    net, cfg, mine, sd = ref_net('config_RefVSR_MFID_8K', t, save_sample=False)
    matches = []
    hook = net.Network.feature_match.register_forward_hook(lambda m, i, o: matches.append((o[0].clone(), o[1].clone())))
    with torch.no_grad():
        for f in range(nframes):
            wi = window_indices(f, clip_n, t)
            del matches[:]
            t0 = time.time()
            res = net(lr[wi][None], rf[wi][None], f == 0, is_log=False, is_train=False)['result']
            assert tuple(res.shape) == (1, 3, s * h, s * w)
            p = float(10 * torch.log10(1 / torch.mean((res - gt[f][None]) ** 2)))
            print('  frame %d: %.1f s, PSNR vs GT %.6f dB' % (f, time.time() - t0, p), flush=True)
            arrs['psnr_%d' % f] = np.float64(p)
            for ci, (y0, x0) in enumerate(crops):
                arrs['crop%d_%d' % (ci, f)] = res[0, :, y0:y0 + 128, x0:x0 + 128].clone()
            arrs['sub_%d' % f] = res[0, :, ::stride, ::stride].clone()
            # feature_match runs for window positions range_start..t-1: the centre frame is call ctr - range_start
            conf, idx = matches[t // 2 if f == 0 else 0]
            arrs['conf_%d' % f] = conf[0, 0, ::4, ::4].clone()          # (bicubic x4 of the matching grid's map, attention.py:96-98)
            arrs['idx_%d' % f] = idx[0].to(torch.int32).clone()
            del res
    hook.remove()
    save(tag, **arrs)


def gen_full_long(nframes=12):
    """The north-star bar itself -- |PSNR(build, GT) - PSNR(reference, GT)| < 1e-3 dB -- over a LONGER full-size stream than the two
    frames of e2e_full_S_270x480_t5 (VERDICT r4 weak 1 iii): config_RefVSR_small_MFID (BASELINE configs[3]'s model: reset_branch = 9, so
    the 12 frames cross a restart of the forward branch), 270 x 480 -> 1080 x 1920, t = 5, random AND 'plausible' weights.  Stored per
    frame: the PSNR scalar and one 64 x 64 crop at output resolution (the fixture stays small).  ~1.5 min per frame and variant."""
    from refvsr_amd.synth import make_clip, window_indices
    import time
    lr, rf, gt = make_clip(nframes, 270, 480, seed=0)
    arrs = dict(nframes=np.int64(nframes), crop=np.asarray([520, 930], np.int64),
                lr_checksum=np.float64(lr.double().sum().item()), ref_checksum=np.float64(rf.double().sum().item()))
    for variant in (None, 'plausible'):
        tag = '' if variant is None else 'p_'
        print('== full-size small_MFID 270x480 t=5, %d frames, weights: %s ==' % (nframes, variant or 'random'), flush=True)
        net, cfg, mine, sd = ref_net('config_RefVSR_small_MFID', 5, save_sample=False)
        assert cfg.reset_branch == 9
        if variant:
            net.load_state_dict(wts.make_state_dict(mine, SEED_W, variant=variant), strict=True)
        with torch.no_grad():
            for f in range(nframes):
                w = window_indices(f, nframes, 5)
                t0 = time.time()
                res = net(lr[w][None], rf[w][None], f == 0, is_log=False, is_train=False)['result']
                p = float(10 * torch.log10(1 / torch.mean((res - gt[f][None]) ** 2)))
                print('  frame %d: %.1f s, PSNR vs GT %.6f dB' % (f, time.time() - t0, p), flush=True)
                arrs[tag + 'psnr_%d' % f] = np.float64(p)
                arrs[tag + 'crop_%d' % f] = res[0, :, 520:584, 930:994].clone()
    save('e2e_full_S_270x480_t5_long', **arrs)


def main():
    if '--full-mfid' in sys.argv:
        os.makedirs(GOLD, exist_ok=True)
        torch.set_num_threads(8)
        gen_full_mfid()
        return
    if '--full-long' in sys.argv:
        os.makedirs(GOLD, exist_ok=True)
        torch.set_num_threads(8)
        gen_full_long()
        return
    if '--full-hd' in sys.argv:
        os.makedirs(GOLD, exist_ok=True)
        torch.set_num_threads(8)
        if '--hd-size' in sys.argv:                       # e.g. --hd-size 540x960 (the fall-back when 62 GB do not hold 1080p)
            hh, ww = sys.argv[sys.argv.index('--hd-size') + 1].split('x')
            gen_full_hd(int(hh), int(ww))
        else:
            gen_full_hd()
        return
    if '--spec' in sys.argv:
        gen_spec()
        return
    if '--plugin-spec' in sys.argv:
        gen_plugin_spec()
        return
    if '--full' in sys.argv:
        os.makedirs(GOLD, exist_ok=True)
        torch.set_num_threads(8)
        gen_full()
        return
    os.makedirs(GOLD, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    E2E = [('S_16x16_t3', 'config_RefVSR_small_L1', 3, 16, 16, 4, 'keep'),
           ('S_18x26_t5', 'config_RefVSR_small_L1', 5, 18, 26, 4, 'keep'),
           ('S_24x32_t5_reset3', 'config_RefVSR_small_L1', 5, 24, 32, 5, 3),
           ('F_16x24_t3', 'config_RefVSR_MFID', 3, 16, 24, 3, 'keep'),
           ('HD_32x48_t3', 'config_RefVSR_small_MFID_8K', 3, 32, 48, 3, 'keep'),
           # 7-frame windows on a 5-frame clip: every window replicates frames at a clip edge (datasets.py:233-234)
           ('S_16x24_t7', 'config_RefVSR_small_L1', 7, 16, 24, 5, 'keep'),
           # BASELINE configs[4] model: C = 48, 30 blocks, flag_HD_in (aa1 scale 4 + align, aa2 scale 8 + align), no reset
           ('HD48_64x96_t3', 'config_RefVSR_MFID_8K', 3, 64, 96, 2, 'keep'),
           # x2 SR (config.scale = 2: matching_ksize 4, VGG19[0:7] matching features, aa1 + aa2 alignment, one pixel shuffle)
           ('S2_16x24_t3', 'config_RefVSR_small_L1', 3, 16, 24, 3, 'keep')]
    IR = [('IR_64x64_t5_reset2', 'config_RefVSR_IR_MFID', 5, 64, 64, 4, 2)]
    if '--only' in sys.argv:                     # regenerate one end-to-end fixture: --only S_16x24_t7
        tag = sys.argv[sys.argv.index('--only') + 1]
        for e in IR:
            if e[0] == tag:
                gen_e2e_ir(*e[:6], reset_override=e[6])
        for e in E2E:
            if e[0] == tag:
                gen_e2e(*e[:6], reset_override=e[6], light=e[0].startswith('HD48'), scale=2 if e[0].startswith('S2_') else 4)
        return
    gen_ops()
    for e in E2E:
        gen_e2e(*e[:6], reset_override=e[6], light=e[0].startswith('HD48'), scale=2 if e[0].startswith('S2_') else 4)
    for e in IR:
        gen_e2e_ir(*e[:6], reset_override=e[6])
    gen_spec()
    gen_plugin_spec()


def gen_spec():
    """state-dict contract checksums (from the reference's own modules) for every config, incl. the two RefVSR_IR ones."""
    sums = {}
    for name in ('config_RefVSR_small_L1', 'config_RefVSR_small_MFID', 'config_RefVSR_L1', 'config_RefVSR_MFID',
                 'config_RefVSR_MFID_8K', 'config_RefVSR_small_MFID_8K', 'config_RefVSR_IR_L1', 'config_RefVSR_IR_MFID'):
        net, cfg, mine, sd = ref_net(name, 5 if 'IR' in name else 3)
        sums[name + '/nparams'] = np.int64(sum(v.numel() for v in net.state_dict().values()))
        sums[name + '/ntensors'] = np.int64(len(net.state_dict()))
        sums[name + '/spec_crc'] = np.int64(wts.spec_checksum(mine))
        sums[name + '/frame_num'] = np.int64(importlib.import_module('configs.' + name).get_config('p', 'm', name).frame_num)
    save('state_spec', **sums)


PLUGIN_CONFIGS = ('config_RefVSR_small_L1', 'config_RefVSR_MFID_8K', 'config_RefVSR_IR_L1')


def gen_plugin_spec():
    """The reference shell's own state dict (models/SRNet.py:SRNet on the reference's own config object): [key, shape, dtype] in
    its order, for the configs tests/test_reference_plugin.py runs the plug-in file with -> tests/golden/plugin_state_dict.json."""
    import json
    from models.SRNet import SRNet
    out = {}
    for name in PLUGIN_CONFIGS:
        cfg = importlib.import_module('configs.' + name).get_config('p', 'm', name)
        cfg.cuda, cfg.device, cfg.dist = False, 'cpu', False
        cfg.network_ref = cfg.network
        sd = SRNet(cfg).eval().state_dict()
        out[name] = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()]
    path = os.path.join(GOLD, 'plugin_state_dict.json')
    with open(path, 'w') as f:                                     # one state-dict entry per line
        f.write('{\n' + ',\n'.join('%s: [\n%s\n]' % (json.dumps(name), ',\n'.join(json.dumps(e) for e in ents))
                                   for name, ents in out.items()) + '\n}\n')
    print('  wrote %-34s %7.1f KB' % ('plugin_state_dict.json', os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
