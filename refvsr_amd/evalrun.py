"""Evaluation harness + `run.py`-compatible CLI for the HIP path.

Counterpart of the reference's eval stack, restated from its behaviour:
  * RealMCVSR folder layout and file listing     -- configs/config.py:120-152, data_loader/utils.py:247-287
  * per-frame sliding windows, edge-frame repeats -- data_loader/datasets.py:222-234
  * `is_first` per clip                            -- datasets.py:286-288 (the reference yields False for frame 0
    of a single-clip dataset and then crashes, RefVSR.py:257-258; here the first frame of every clip is True)
  * PSNR = 10 log10(1/mse)                         -- trainers/trainer.py:252-254
  * flag_HD_in configs (result = scale x the ground truth): both scores on the bicubic down-scale of the result -- PSNR of the
    clamped image (models/loss/Loss.py:91-92,141), SSIM of the unclamped one (evaluation/eval_qual_quan.py:85-92)
  * SSIM = skimage.structural_similarity defaults  -- evaluation/metrics.py:17-18 (7x7 uniform window, sample
    covariance, K1=0.01, K2=0.03, mean over channels) re-implemented (skimage is not in this image)
  * score file lines / output tree                 -- evaluation/eval_qual_quan.py:98-101,106-124,140-143
  * `--eval_mode quan_FOV` (eval.py:16-21): PSNR / SSIM inside, outside and in rings around the overlapped field of view
    -- evaluation/eval_quan_FOV.py:155-192 (the 16 masked scores per frame), :93-111, :196, :245-264 (its lines and blocks)
  * `--eval_mode quan_conf_map` (eval.py:16-21): the four confidence maps that steer the fusion, min/max-normalised and coloured with
    matplotlib's inferno, as images next to the input and the result -- evaluation/eval_quan_conf_map.py:64-100,148-165 (the maps, on
    the device here: ops.conf_colormap), :47,115,179 (its lines)
  * checkpoint loading (flat state dict, optional `module.` prefix) -- ckpt_manager.py:50-60

    python -m refvsr_amd.evalrun --mode amp_RefVSR_small_L1 --config config_RefVSR_small_L1 --data RealMCVSR \
        --ckpt_abs_name ckpt/RefVSR_small_L1.pytorch --data_offset /data --output_offset ./result --frame_num 5
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

from .config import get_config, set_data_path
from .synth import window_indices


# ------------------------------------------------------------------------------------------------ data
def load_file_list(root_path):
    """Leaf folders under root_path (sorted) and their sorted files (data_loader/utils.py:247-287)."""
    folders, files = [], []
    for root, dirnames, filenames in os.walk(root_path):
        dirnames[:] = [d for d in dirnames if not d.startswith('@')]
        if not dirnames:
            fs = sorted(os.path.join(root, f) for f in filenames if not f.startswith('.') and f != 'Thumbs.db')
            folders.append(root)
            files.append(fs)
    order = np.argsort(np.array(folders)) if folders else []
    return [folders[i] for i in order], [files[i] for i in order]


def read_frame(path, dtype='float32'):
    """PIL image -> float32 [3,H,W] in [0,1] (data_loader/utils.py:12-41), or (dtype 'uint8', extension) the decoded bytes as a uint8
    [3,H,W] channels-last view of the [H,W,3] array: the network converts them on the device, bit-identical to the float32 frame."""
    from PIL import Image
    if dtype == 'uint8':
        return torch.from_numpy(np.array(Image.open(path).convert('RGB'), dtype=np.uint8)).permute(2, 0, 1)
    a = np.asarray(Image.open(path).convert('RGB'), dtype=np.float32) / 255.0
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def stack_frames(frames):
    """torch.stack for the loader's frames: uint8 channels-last frames stay channels-last ([.., h, w, 3] bytes underneath), the layout
    the network takes without a copy."""
    if frames[0].dtype == torch.uint8:
        return torch.stack([f.movedim(-3, -1) for f in frames]).movedim(-1, -3)
    return torch.stack(frames)


def write_frame(path, img, quality=None):
    from PIL import Image
    if img.dtype == torch.uint8:
        # config.result_dtype = 'uint8': the output head stored rint(255 x) itself (REFVSR_RESULT_U8) -- the bytes computed below
        # (config.result_layout = 'hwc': the transposed view is the dense array itself, no strided copy in fromarray)
        im = Image.fromarray(img.detach().cpu().numpy().transpose(1, 2, 0))
    else:
        a = (img.detach().float().cpu().clamp(0, 1).numpy().transpose(1, 2, 0) * 255.0)
        # cv2.imwrite converts a float image with convertTo(CV_8U) = saturate_cast<uchar>: round to nearest, saturate
        # (eval_qual_quan.py:117-119 hands it output*255 as float)
        im = Image.fromarray(np.rint(a).clip(0, 255).astype(np.uint8))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    im.save(path, **({'quality': quality} if quality else {}))


class ClipSet(object):
    """One item per output frame of every clip, in the reference's order (datasets.py:150-316)."""

    def __init__(self, config):
        self.config = config
        E = config.EVAL
        _, self.lr_uw = load_file_list(os.path.join(E.LR_data_path, config.UW_path))
        _, self.lr_w = load_file_list(os.path.join(E.LR_data_path, config.W_path))
        _, self.hr_uw = load_file_list(os.path.join(E.HR_data_path, config.UW_path))
        assert len(self.lr_uw) == len(self.lr_w) == len(self.hr_uw) and self.lr_uw, \
            'no clips found under %s' % E.LR_data_path
        self.items = [(v, f) for v in range(len(self.lr_uw)) for f in range(len(self.lr_uw[v]))]
        self.input_dtype = str(getattr(config, 'input_dtype', None) or 'float32')
        # --metrics device: the ground truth stays the decoded bytes (the device scorer looks them up: T[u] == the float32 frame)
        self.gt_dtype = 'uint8' if getattr(E, 'metrics', 'host') == 'device' else 'float32'
        self._cache = {}

    def __len__(self):
        return len(self.items)

    def _frame(self, path, dtype=None):
        dtype = dtype or self.input_dtype
        if (path, dtype) not in self._cache:
            if len(self._cache) > 64:
                self._cache.clear()
            self._cache[(path, dtype)] = read_frame(path, dtype)
        return self._cache[(path, dtype)]

    def __getitem__(self, index):
        v, f = self.items[index]
        t = self.config.frame_num
        n = len(self.lr_uw[v])
        win = window_indices(f, n, t)
        name = os.path.basename(os.path.dirname(self.lr_uw[v][f]))
        vid_filter = getattr(self.config.EVAL, 'vid_name', None)
        if vid_filter is not None and name not in vid_filter:
            return {'is_continue': True, 'is_first': True, 'video_name': name, 'frame_len': n}
        return {
            'LR_UW': stack_frames([self._frame(self.lr_uw[v][i]) for i in win]),
            'LR_REF_W': stack_frames([self._frame(self.lr_w[v][i]) for i in win]),
            'HR_UW': self._frame(self.hr_uw[v][f], self.gt_dtype),      # (the scores' ground truth stays float on the host path)
            'is_first': f == 0, 'video_name': name, 'video_idx': v, 'video_len': len(self.lr_uw),
            'frame_idx': f, 'frame_len': n, 'frame_name': os.path.basename(self.lr_uw[v][f]),
            'frame_ids': [(v, int(i)) for i in win],     # names the window's frames for the cross-window cache
        }


# ------------------------------------------------------------------------------------------------ metrics
def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / torch.mean((a.float() - b.float()) ** 2)))


def ssim(a, b, data_range=1.0, win=7):
    """skimage.metrics.structural_similarity(a, b, data_range=1.0, multichannel=True) for [3,H,W] tensors."""
    a, b = a.double()[None], b.double()[None]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    norm = win * win / (win * win - 1.0)
    f = lambda x: F.avg_pool2d(x, win, stride=1)
    ua, ub = f(a), f(b)
    va, vb, vab = norm * (f(a * a) - ua * ua), norm * (f(b * b) - ub * ub), norm * (f(a * b) - ua * ub)
    s = ((2 * ua * ub + c1) * (2 * vab + c2)) / ((ua * ua + ub * ub + c1) * (va + vb + c2))
    return float(s.mean())


# ------------------------------------------------------------------------------------------------ eval loop
def load_checkpoint(net, path):
    sd = torch.load(path, map_location='cpu')
    if isinstance(sd, dict) and 'state_dict' in sd:
        sd = sd['state_dict']
    return net.load_state_dict(sd, strict=False)


def evaluate(config, net=None, log=print):
    """eval_qual_quan counterpart.  Returns dict(psnr=[..], ssim=[..], frames=N, seconds=[..]).
    'FOV' in EVAL.eval_mode: eval_quan_FOV counterpart -- the same loop; a frame's score is its FOV table (metrics.fov_table,
    [6 keys][fi, fo, fr][psnr, ssim]), whose key 1 fi pair is the per-frame line; the summaries are the reference's six-row blocks; no
    image is written (the reference has that part commented out); the tables are returned as res['fov'].
    'conf_map' in EVAL.eval_mode: eval_quan_conf_map counterpart -- the same loop without scores (psnr / ssim stay empty; --metrics,
    -qualitative_only and -quantitative_only have no effect, as in the reference's loop): per frame the input, the result and the four
    maps of 'eval_vis' coloured by ONE ops.conf_colormap launch per network call (CONF_MAP_DIRS names the folders); with --frame_group
    G > 1 the maps come from forward_group(want_conf=True).  RefVSR_IR has no such maps (the reference fails on None['conf_map'])."""
    if 'conf_map' in str(config.EVAL.eval_mode) and config.network == 'RefVSR_IR':
        raise RuntimeError('--eval_mode %s: RefVSR_IR returns no confidence maps (config %s)' % (config.EVAL.eval_mode, config.get('config')))
    from . import SRNet
    E = config.EVAL
    fov = 'FOV' in str(E.eval_mode)
    conf = 'conf_map' in str(E.eval_mode)
    if conf:
        config.save_sample = True            # eval_quan_conf_map.py:23: Network.forward(is_log=True) then returns 'eval_vis'
    video = getattr(E, 'video_out', None)
    if video and (fov or conf):
        raise RuntimeError(VIDEO_MODE_MESSAGE % E.eval_mode)
    if video and video != 'y4m':
        raise RuntimeError("--video_out: 'y4m' is the only container (got %r)" % (video,))
    if video and getattr(config, 'result_yuv', None) not in ('i420', 'i420p10'):
        raise RuntimeError("--video_out y4m needs config.result_yuv = 'i420' | 'i420p10' (Y4M frames are planar), got %r" % (getattr(config, 'result_yuv', None),))
    if fov and config.flag_HD_in:
        raise RuntimeError('--eval_mode %s: flag_HD_in configs are not supported (the reference scores a cv2.resize(INTER_CUBIC) of the result)' % E.eval_mode)
    if net is None:
        if config.device != 'cuda':
            raise RuntimeError('refvsr_amd has no CPU path; run on the GPU (drop --cpu)')
        net = SRNet(config).to('cuda').eval()
        if E.ckpt_abs_name:
            log('Loading checkpoint %s: %s' % (E.ckpt_abs_name, load_checkpoint(net, E.ckpt_abs_name)))
    if conf:
        net.Network.config.save_sample = True            # (a caller's net may carry a config of its own)
    ckpt_name = os.path.basename(E.ckpt_abs_name) if E.ckpt_abs_name else 'seeded'
    date = datetime.datetime.now().strftime('%Y_%m_%d_%H%M')
    root = os.path.join(E.LOG_DIR.save, E.eval_mode, ckpt_name.split('.')[0])
    out_root = os.path.join(root, E.data, date)
    os.makedirs(root, exist_ok=True)
    score_path = os.path.join(root, 'score_%s_%s.txt' % (E.data, E.eval_mode))
    ds = ClipSet(config)
    dev = next(net.parameters()).device
    res = {'psnr': [], 'ssim': [], 'seconds': [], 'frames': 0}
    if fov:
        res['fov'] = []
    # --frame_group G (extension, default 1 = the reference's loop): G consecutive windows of a clip per network call
    # (SRNet.forward_group: the backward branches of the G frames as multi-map launches; results bit-identical); the per-frame time in
    # the score lines is then the group's time / G
    G = max(1, int(getattr(E, 'frame_group', 1) or 1))
    # (the state to restore is the net's own: a caller's net may have been switched on without config.pipelined saying so)
    engines = getattr(net.Network, '_engines', None)
    was_pipelined = bool(engines[0].pipelined) if engines else bool(getattr(config, 'pipelined', False))
    if G > 1:
        net.Network.set_pipelined(True)          # (restored at the end: the caller's plain net(...) calls keep their stream contract)
    st = {'clip_p': 0.0, 'clip_s': 0.0, 'clip_t': 0.0, 'clip_n': 0, 'first_line': True, 'prev': None, 'clip_fov': 0.0, 'video': None, 'video_clip': None}
    # --metrics device (extension, default 'host' = the loop below as it always was): the scores come from ONE refvsr_score_frames launch
    # per network call, on the caller's current stream (which already waits for the results, pipelined mode included: INTEGRATION.md),
    # and cross to the host as 16 bytes per frame; the frame itself is only copied when an image is written
    on_device = getattr(E, 'metrics', 'host') == 'device' and not getattr(E, 'qualitative_only', False) and not conf

    def score_device(outs, items):
        from . import ops
        from .metrics import psnr_from_mse
        gts = [it['HR_UW'].to(dev) for it in items]              # (decoded bytes, channels-last: a quarter of the float frame)
        # flag_HD_in: the result is `scale` times the ground truth and the scores are those of its bicubic down-scale, which the
        # kernel forms while it stages its tiles (refvsr_score_frames_down): the big frame is read once where it lies
        down = int(config.scale) if config.flag_HD_in else 1     # (no FOV mode here: evaluate() refuses it for these configs)
        for o, g in zip(outs, gts):
            if tuple(o[0].shape) != (3, down * g.shape[-2], down * g.shape[-1]):
                raise RuntimeError('--metrics device: result %s and ground truth %s differ in shape' % (tuple(o[0].shape), tuple(g.shape)))
        if fov:
            # one refvsr_score_regions launch: 7 rectangles x 16 bytes per frame cross to the host
            from .metrics import fov_rects, fov_table
            h, w = gts[0].shape[-2:]
            sums = ops.score_regions([o[0] for o in outs], gts, fov_rects(h, w)).cpu().numpy()
            tables = [fov_table(sm, h, w) for sm in sums]
            return [(float(t[0, 0, 0]), float(t[0, 0, 1]), t) for t in tables]
        if down == 1:
            sc = ops.score_frames([o[0] for o in outs], gts, win=7).cpu().tolist()
        else:
            sc = ops.score_frames([o[0] for o in outs], gts, win=7, down=down).cpu().tolist()
        return [(psnr_from_mse(m), s) for m, s in sc]

    def colour(vis_list):
        """The windows' 'eval_vis' dicts -> per window {folder: uint8 [h, w, 3] on the host}: one conf_colormap launch for all maps."""
        from . import ops
        maps = [v[src] for v in vis_list for _, src in CONF_MAP_DIRS]
        imgs = [x.cpu() for x in ops.conf_colormap(maps)]
        k = len(CONF_MAP_DIRS)
        return [dict((CONF_MAP_DIRS[j][0], imgs[b * k + j]) for j in range(k)) for b in range(len(vis_list))]

    def write_video(it, y):
        """--video_out y4m (extension): the frame's 'yuv' [1, 3sh/2, sw] -- 1.5 samples per pixel cross to the host -- appended to
        <out_root>/y4m/<clip>.y4m, one file per clip."""
        from .yuv import Y4MWriter
        a = y[0].cpu().numpy()
        if st['video_clip'] != it['video_name']:
            close_video()
            path = os.path.join(out_root, 'y4m', '%s.y4m' % it['video_name'])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            st['video'] = Y4MWriter(path, a.shape[0] * 2 // 3, a.shape[1], config.result_yuv, getattr(E, 'video_fps', None) or (30, 1),
                                    getattr(config, 'yuv_range', None) or 'limited')
            st['video_clip'] = it['video_name']
            res.setdefault('videos', []).append(path)
        st['video'].write(a)

    def close_video():
        if st['video'] is not None:
            st['video'].close()
        st['video'] = st['video_clip'] = None

    def emit_conf(it, out, lr_c, dt, imgs):
        out_raw = out[0].cpu()
        out_cpu = out_raw.float() / 255.0 if out_raw.dtype == torch.uint8 else out_raw.float()
        line = '[EVAL {}|{}|{}][{}/{}][{}/{}] {} ({:.5f}sec)'.format(
            config.mode, E.data, it['video_name'], it['video_idx'] + 1, it['video_len'], it['frame_idx'] + 1, it['frame_len'],
            it['frame_name'], dt)
        log(line)
        with open(score_path, 'w' if st['first_line'] else 'a') as fh:
            fh.write(line + '\n')
        st['first_line'] = False
        stem = it['frame_name'].split('.')[0]
        for fmt in ('png', 'jpg'):
            base = os.path.join(out_root, fmt)
            write_frame(os.path.join(base, 'input', it['video_name'], '%s.%s' % (stem, fmt)), lr_c)
            write_frame(os.path.join(base, 'output', it['video_name'], '%s.%s' % (stem, fmt)), out_raw if out_raw.dtype == torch.uint8 else out_cpu)
            for folder, _ in CONF_MAP_DIRS:
                write_frame(os.path.join(base, folder, it['video_name'], '%s.%s' % (stem, fmt)), imgs[folder].permute(2, 0, 1))
        st['clip_t'] += dt
        st['clip_n'] += 1
        st['prev'] = it
        res['seconds'].append(dt)
        res['frames'] += 1

    def emit(it, out, lr_c, dt, scored=None, vis=None, yuv=None):
        if video:
            write_video(it, yuv)
        if conf:
            return emit_conf(it, out, lr_c, dt, scored if scored is not None else colour([vis])[0])
        if on_device and scored is None:
            scored = score_device([out], [it])[0]
        if scored is not None and (fov or getattr(E, 'quantitative_only', False)):
            out_raw = out_cpu = None                 # (nothing reads the frame: it stays on the device)
        else:
            out_raw = out[0].cpu()
            # (result_dtype 'uint8' / 'float16', extensions: the scores are then those of the quantised frame; the PNG bytes are the same)
            out_cpu = out_raw.float() / 255.0 if out_raw.dtype == torch.uint8 else out_raw.float()
        p = s = 0.0
        table = None
        if scored is not None:
            p, s = scored[:2]
            table = scored[2] if fov else None
        elif fov:
            from .metrics import fov_scores_host
            gt = it['HR_UW']
            out_cpu = out_cpu.contiguous()           # (host scores are taken on the planar frame whatever --result_layout says)
            if out_cpu.shape != gt.shape:
                raise RuntimeError('--eval_mode %s: result %s and ground truth %s differ in shape' % (E.eval_mode, tuple(out_cpu.shape), tuple(gt.shape)))
            table = fov_scores_host(out_cpu, gt)
            p, s = float(table[0, 0, 0]), float(table[0, 0, 1])
        elif not getattr(E, 'qualitative_only', False):
            gt = it['HR_UW']
            sc_cpu = out_cpu.contiguous()            # (host scores are taken on the planar frame whatever --result_layout says)
            if config.flag_HD_in:
                # the result is `scale` times the ground truth; both scores are those of its bicubic down-scale: the PSNR of the
                # clamped image (models/loss/Loss.py:91-92,141), the SSIM of the unclamped one (eval_qual_quan.py:85-92, whose
                # cv2.resize(INTER_CUBIC) is this filter at an exact integer factor)
                d = F.interpolate(sc_cpu[None], scale_factor=1.0 / config.scale, mode='bicubic', align_corners=False)[0]
                p = psnr(d.clamp(0, 1), gt)
                s = ssim(d, gt)
            else:
                p = psnr(sc_cpu, gt)
                s = ssim(sc_cpu, gt)
        line = '[EVAL {}|{}|{}][{}/{}][{}/{}] {} PSNR: {:.5f} SSIM: {:.5f} ({:.5f}sec)'.format(
            config.mode, E.data, it['video_name'], it['video_idx'] + 1, it['video_len'], it['frame_idx'] + 1,
            it['frame_len'], it['frame_name'], p, s, dt)
        log(line)
        with open(score_path, 'w' if st['first_line'] else 'a') as fh:
            fh.write(line + '\n')
        st['first_line'] = False
        if not fov and not getattr(E, 'quantitative_only', False):
            stem = it['frame_name'].split('.')[0]
            for fmt in ('png', 'jpg'):
                base = os.path.join(out_root, fmt)
                write_frame(os.path.join(base, 'input', it['video_name'], '%s.%s' % (stem, fmt)), lr_c)
                write_frame(os.path.join(base, 'output', it['video_name'], '%s.%s' % (stem, fmt)), out_raw if out_raw.dtype == torch.uint8 else out_cpu)
        st['clip_p'] += p
        st['clip_s'] += s
        st['clip_t'] += dt
        st['clip_n'] += 1
        st['prev'] = it
        if fov:
            st['clip_fov'] = st['clip_fov'] + table
            res['fov'].append(table)
        res['psnr'].append(p)
        res['ssim'].append(s)
        res['seconds'].append(dt)
        res['frames'] += 1

    def flush(pending, first=False):
        if not pending:
            return
        t0 = time.time()
        lrs, rfs = (stack_frames([it[k] for it in pending]).to(dev) for k in ('LR_UW', 'LR_REF_W'))
        if lrs.dtype != torch.uint8:
            lrs, rfs = lrs.float().contiguous(), rfs.float().contiguous()
        kw = {'want_conf': True} if conf else {}
        got = net.forward_group(lrs, rfs, [it['frame_ids'] for it in pending], is_first_frame=first, **kw)
        outs = got['result']
        torch.cuda.synchronize()
        dt = (time.time() - t0) / len(pending)
        c = lrs.shape[1] // 2
        if conf:
            scored = colour(got['eval_vis'])         # (the windows' images, in the place of their scores)
        else:
            scored = score_device(outs, pending) if on_device else [None] * len(pending)
        for b, it in enumerate(pending):
            emit(it, outs[b], lrs[b, c], dt, scored[b], yuv=got['yuv'][b] if video else None)
        del pending[:]

    def clip_summary():
        """The clip's MEAN line / block, named for the clip it summarises; resets the clip's sums."""
        if st['clip_n']:
            n = st['clip_n']
            if fov:
                _fov_clip_summary(config, score_path, st['prev'], st['clip_fov'] / n, st['clip_t'] / n, log)
            elif conf:
                _conf_clip_summary(config, score_path, st['prev'], st['clip_t'] / n, log)
            else:
                _clip_summary(config, score_path, st['prev'], st['clip_p'], st['clip_s'], st['clip_t'], n, log)
        st['clip_p'] = st['clip_s'] = st['clip_t'] = st['clip_fov'] = 0.0
        st['clip_n'] = 0

    try:
        _evaluate_loop(net, ds, dev, E, G, st, emit, flush, clip_summary, conf)
    finally:
        close_video()
        if G > 1 and not was_pipelined:
            torch.cuda.synchronize()
            net.Network.set_pipelined(False)
    clip_summary()
    n = max(res['frames'], 1)
    if fov:
        total = fov_block('\n[TOTAL {}|{}] \n'.format(ckpt_name, E.data), sum(res['fov']) / n if res['fov'] else np.zeros((6, 3, 2)),
                          ') ({:.5f}sec)\n\n'.format(sum(res['seconds']) / n))
        log(total)
        with open(score_path, 'a') as fh:
            fh.write(total)
    elif conf:
        total = '\n[TOTAL {}|{}] ({:.5f}sec)'.format(ckpt_name, E.data, sum(res['seconds']) / n)
        log(total)
        with open(score_path, 'a') as fh:
            fh.write(total + '\n')
    else:
        total = '\n[TOTAL {}|{}] PSNR: {:.5f} SSIM: {:.5f} ({:.5f}sec)'.format(
            ckpt_name, E.data, sum(res['psnr']) / n, sum(res['ssim']) / n, sum(res['seconds']) / n)
        log(total)
        with open(score_path, 'a') as fh:
            fh.write(total + '\n')
    res['score_file'], res['output_root'] = score_path, out_root
    return res


def _evaluate_loop(net, ds, dev, E, G, st, emit, flush, clip_summary, conf=False):
    """The per-frame loop of evaluate() (eval_qual_quan.py:39-128, eval_quan_FOV.py:55-232, eval_quan_conf_map.py:32-174): emit scores
    and logs a frame, clip_summary closes a clip.  conf: a one-window call is the reference's own, net(.., is_log=True), whose
    'eval_vis' goes to emit; in a grouped run every call is a forward_group, a clip's first frame one of a single window."""
    with torch.no_grad():
        pending = []
        for i in range(len(ds)):
            it = ds[i]
            if it.get('is_continue'):
                continue
            if it['is_first']:
                flush(pending)
                clip_summary()
                net.Network.reset()
            use_ids = getattr(E, 'use_frame_ids', True) and 'frame_ids' in it
            if G > 1 and use_ids and conf and it['is_first']:
                flush([it], first=True)
                continue
            if G > 1 and use_ids and not it['is_first']:
                pending.append(it)
                if len(pending) == G:
                    flush(pending)
                continue
            t0 = time.time()
            lr, rf = it['LR_UW'][None].to(dev), it['LR_REF_W'][None].to(dev)
            kw = {'frame_ids': it['frame_ids']} if use_ids else {}
            got = net(lr, rf, it['is_first'], is_log=conf, is_train=False, **kw)
            torch.cuda.synchronize()
            emit(it, got['result'], lr[0, lr.shape[1] // 2], time.time() - t0, vis=got['eval_vis'] if conf else None, yuv=got.get('yuv'))
        flush(pending)


def _clip_summary(config, score_path, it, p, s, t, n, log):
    line = '[MEAN EVAL {}|{}|{}][{}/{}] PSNR: {:.5f} SSIM: {:.5f} ({:.5f}sec)\n'.format(
        config.mode, config.EVAL.data, it['video_name'], it['video_idx'], it['video_len'], p / n, s / n, t / n)
    log(line)
    with open(score_path, 'a') as fh:
        fh.write(line + '\n')


# folder of the reference's output tree <- key of 'eval_vis' (eval_quan_conf_map.py:64-77,148-165)
CONF_MAP_DIRS = (('conf_map_norm', 'conf_map'), ('conf_map_prop_norm', 'conf_map_prop'),
                 ('conf_map_prop_b_norm', 'conf_map_prop_backward'), ('conf_map_prop_f_norm', 'conf_map_prop_forward'))


def _conf_clip_summary(config, score_path, it, t, log):
    line = '[MEAN EVAL {}|{}|{}][{}/{}] ({:.5f}sec)\n'.format(config.mode, config.EVAL.data, it['video_name'], it['video_idx'], it['video_len'], t)
    log(line)
    with open(score_path, 'a') as fh:
        fh.write(line + '\n')


def fov_block(head, table, tail):
    """The six labelled rows of a FOV summary (eval_quan_FOV.py:93-111 / :245-264, its format strings) between `head` and `tail`;
    table: [6 keys][fi, fo, fr][psnr, ssim]."""
    from .metrics import FOV_KEYS as keys
    out = head
    for m, name in enumerate(('PSNR', 'SSIM')):
        out += (')\n' if m else '') + '[%s-FOV_in  ] (' % name
        for k, v in zip(keys, table[:, 0, m]):
            out += '0-{:3.1f}%: {:.5f}, '.format(k * 100, v)
        out += ')\n[%s-FOV_out ] (' % name
        for k, v in zip(keys, table[:, 1, m]):
            out += '{:3.1f}-100%: {:.5f}, '.format(k * 100, v)
        out += ')\n[%s-FOV_ring] (' % name
        for k, v in zip(keys, table[:, 2, m]):
            out += '{:3.1f}-{:3.1f}%: {:.5f}, '.format(keys[-1] * 100, k * 100, v)
    return out + tail


def _fov_clip_summary(config, score_path, it, table, t, log):
    block = fov_block('[MEAN EVAL {}|{}|{}][{}/{}] ({:.5f}sec) \n'.format(config.mode, config.EVAL.data, it['video_name'], it['video_idx'],
                                                                         it['video_len'], t), table, ') \n\n')
    log(block)
    with open(score_path, 'a') as fh:
        fh.write(block)


VIDEO_MODE_MESSAGE = ("--video_out writes the frames of the qual_quan loop; --eval_mode %s writes no result video (drop --video_out)")


# ------------------------------------------------------------------------------------------------ CLI
def build_config(argv=None):
    """run.py:218-417 flag surface (evaluation subset)."""
    ap = argparse.ArgumentParser(description='RefVSR evaluation on the MI355X HIP path')
    ap.add_argument('-proj', '--project', type=str, default='RefVSR_CVPR2022')
    ap.add_argument('-m', '--mode', type=str, default='eval')
    ap.add_argument('-c', '--config', type=str, default='config_RefVSR_small_L1')
    ap.add_argument('-data', '--data', type=str, default='RealMCVSR')
    ap.add_argument('-net', '--network', type=str, default=None)
    ap.add_argument('-data_offset', '--data_offset', type=str, default=None)
    ap.add_argument('-output_offset', '--output_offset', type=str, default='./result')
    ap.add_argument('-ckpt_abs_name', '--ckpt_abs_name', type=str, default=None)
    ap.add_argument('-cpu', '--cpu', action='store_true')
    ap.add_argument('-eval_mode', '--eval_mode', type=str, default='qual_quan',
                    help="'qual_quan' (whole-frame PSNR / SSIM and result images) | a name with 'FOV' in it, e.g. 'quan_FOV': PSNR / SSIM "
                         "inside, outside and in rings around the overlapped field of view, no images (with --metrics device one "
                         "refvsr_score_regions launch per network call) | a name with 'conf_map' in it, e.g. 'quan_conf_map': no "
                         "scores; the input, the result and the four confidence maps of the fusion as inferno-coloured images (one "
                         "refvsr_conf_colormap launch per network call; not for RefVSR_IR)")
    ap.add_argument('-test_set', '--test_set', type=str, default='test')
    ap.add_argument('-qualitative_only', '--qualitative_only', action='store_true')
    ap.add_argument('-quantitative_only', '--quantitative_only', action='store_true')
    ap.add_argument('-is_gradio', '--is_gradio', action='store_true')
    ap.add_argument('-frame_num', '--frame_num', type=int, default=None)
    ap.add_argument('-vid_name', '--vid_name', nargs='+', default=None)
    ap.add_argument('-ss', '--save_sample', action='store_true')
    ap.add_argument('--frame_group', type=int, default=1, help='extension: consecutive frames of a clip per network call (1 = the reference loop; 4 = '
                                                                'multi-map launches of the backward branches, same results)')
    ap.add_argument('--result_dtype', default='float32', choices=['float32', 'float16', 'uint8'],
                    help="extension: what the output head stores ('uint8' = rint(255 x), the bytes of the written PNG; the scores are then "
                         "those of the quantised frame)")
    ap.add_argument('--result_layout', default='chw', choices=['chw', 'hwc'],
                    help="extension: memory layout of the result frames ('hwc' = the output head stores them interleaved, dense [h, w, 3] "
                         "under the unchanged [3, h, w] shape: the image writer gets its array without a host-side transposition; same "
                         "scores and image bytes)")
    ap.add_argument('--input_dtype', default='float32', choices=['float32', 'uint8'],
                    help="extension: what the loader hands the network ('uint8' = the decoded bytes, converted exactly on the device: "
                         "a quarter of the bytes in host memory and across PCIe; same scores and PNG bytes)")
    ap.add_argument('--weight_precision', default='hi_lo', choices=['hi_lo', 'fp16', 'amp'],
                    help="extension: conv weights of the engine ('fp16' = the reference's fp16-autocast arithmetic, mid_channels = 24 "
                         "models only; 'amp' = 'fp16' where the config sets is_amp)")
    ap.add_argument('--weight_check', default='auto', choices=['auto', 'sync', 'off'],
                    help="extension: when the packed weights are checked against a device fingerprint of the parameters ('auto' = "
                         "synchronously where the host waits anyway or a clip starts, asynchronously in steady state; 'sync' = every call; "
                         "'off' = the host-side detector alone)")
    ap.add_argument('--metrics', default='host', choices=['host', 'device'],
                    help="extension: where PSNR / SSIM are computed ('device' = one refvsr_score_frames launch per network call in float64, "
                         "16 bytes per frame cross to the host and with --quantitative_only the frame never does; SSIM agrees with the host "
                         "to 1e-10, PSNR to 2e-5 dB -- the host's mean is float32 -- so a score line may differ in the fifth decimal of PSNR; "
                         "the flag_HD_in configs (.._8K), whose result is `scale` times the ground truth, are scored on the result's bicubic "
                         "down-scale -- PSNR of the clamped, SSIM of the unclamped image -- which 'device' fuses into the same launch "
                         "(refvsr_score_frames_down, float64 taps) and 'host' takes from F.interpolate in float32: SSIM then agrees to ~1e-9)")
    ap.add_argument('--video_out', default=None, choices=['y4m'],
                    help="extension: also write the results as video, one <out_root>/y4m/<clip>.y4m per clip; the frames are converted to "
                         "Y'CbCr 4:2:0 on the device (one refvsr_result_to_yuv420 launch per network call) and 1.5 samples per pixel are "
                         "copied to the host; scores, images and score files are unchanged (not with the FOV / conf_map eval modes)")
    ap.add_argument('--video_fps', default='30', help="extension: frame rate of --video_out, N or N:D (e.g. 30000:1001)")
    ap.add_argument('--video_depth', type=int, default=8, choices=[8, 10], help='extension: bits per sample of --video_out (8: C420jpeg, 10: C420p10)')
    ap.add_argument('--yuv_matrix', default='bt709', choices=['bt709', 'bt601'], help='extension: luma coefficients of --video_out')
    ap.add_argument('--yuv_range', default='limited', choices=['limited', 'full'], help='extension: code range of --video_out')
    args, _ = ap.parse_known_args(argv)
    if args.video_out and ('FOV' in str(args.eval_mode) or 'conf_map' in str(args.eval_mode)):
        raise RuntimeError(VIDEO_MODE_MESSAGE % args.eval_mode)
    from .yuv import parse_fps
    video_fps = parse_fps(args.video_fps)
    cfg = get_config(args.project, args.mode, args.config, args.data)
    if args.video_out:
        cfg.yuv_matrix, cfg.yuv_range = args.yuv_matrix, args.yuv_range
        cfg.result_yuv = 'i420' if args.video_depth == 8 else 'i420p10'
    cfg.result_dtype = args.result_dtype
    cfg.result_layout = args.result_layout
    cfg.weight_precision = args.weight_precision
    cfg.weight_check = args.weight_check
    cfg.input_dtype = args.input_dtype
    if args.network:
        cfg.network = args.network
    if args.frame_num:
        cfg.frame_num = args.frame_num
    cfg.center_idx = cfg.frame_num // 2
    E = cfg.EVAL
    E.ckpt_abs_name = args.ckpt_abs_name
    E.qualitative_only, E.quantitative_only = args.qualitative_only, args.quantitative_only
    E.is_gradio, E.vid_name = args.is_gradio, args.vid_name
    E.eval_mode, E.test_set, E.data = args.eval_mode, args.test_set, args.data
    E.frame_group = args.frame_group
    E.metrics = args.metrics
    E.video_out, E.video_fps = args.video_out, video_fps
    cfg.save_sample = args.save_sample or 'conf_map' in str(args.eval_mode)      # (eval_quan_conf_map.py:23)
    cfg.device = 'cpu' if args.cpu else 'cuda'
    cfg.cuda = not args.cpu
    if args.data_offset:
        cfg.data_offset = args.data_offset
    E.LOG_DIR = {'save': args.output_offset}
    return set_data_path(cfg, E.data, is_train=False)


def main(argv=None):
    cfg = build_config(argv)
    res = evaluate(cfg)
    return 0 if res['frames'] else 1


if __name__ == '__main__':
    sys.exit(main())
