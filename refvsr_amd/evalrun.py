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
import collections
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


# folder of the reference's output tree <- key of 'eval_vis' (eval_quan_conf_map.py:64-77,148-165)
CONF_MAP_DIRS = (('conf_map_norm', 'conf_map'), ('conf_map_prop_norm', 'conf_map_prop'),
                 ('conf_map_prop_b_norm', 'conf_map_prop_backward'), ('conf_map_prop_f_norm', 'conf_map_prop_forward'))

VIDEO_MODE_MESSAGE = ("--video_out writes the frames of the qual_quan loop; --eval_mode %s writes no result video (drop --video_out)")


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


# A frame's score is a pair (v, maps): v a float64 array whose first two numbers are the PSNR / SSIM of the frame's line -- [psnr, ssim],
# a FOV table, or empty (no scores) -- which is also what a clip and the run sum up; maps {folder: uint8 [h, w, 3]}, the frame's
# confidence images (conf_map mode alone).
def _scores_tail(v):
    return 'PSNR: {:.5f} SSIM: {:.5f} '.format(v.flat[0], v.flat[1]) if v.size else ''


def _line_summary(head, v, t, total):
    """One line (eval_qual_quan.py:106-124,140-143; eval_quan_conf_map.py:115,179): a clip's ends in a newline, the run's begins with one."""
    body = '{} {}({:.5f}sec)'.format(head, _scores_tail(v), t)
    return '\n' + body if total else body + '\n'


def _fov_summary(head, v, t, total):
    """The reference's six-row block (eval_quan_FOV.py:93-111 a clip's, :245-264 the run's)."""
    if total:
        return fov_block('\n{} \n'.format(head), v, ') ({:.5f}sec)\n\n'.format(t))
    return fov_block('{} ({:.5f}sec) \n'.format(head, t), v, ') \n\n')


def _host_scores(run, frame, it):
    """PSNR / SSIM of the planar float frame on the host (whatever --result_layout says); -qualitative_only: zeros, as the line prints."""
    if run.qualitative_only:
        return np.zeros(2)
    gt, frame = it['HR_UW'], frame.contiguous()
    if run.config.flag_HD_in:
        # the result is `scale` times the ground truth; both scores are those of its bicubic down-scale: the PSNR of the clamped image
        # (models/loss/Loss.py:91-92,141), the SSIM of the unclamped one (eval_qual_quan.py:85-92, whose cv2.resize(INTER_CUBIC) is this
        # filter at an exact integer factor)
        d = F.interpolate(frame[None], scale_factor=1.0 / run.config.scale, mode='bicubic', align_corners=False)[0]
        return np.array([psnr(d.clamp(0, 1), gt), ssim(d, gt)])
    return np.array([psnr(frame, gt), ssim(frame, gt)])


def _host_fov(run, frame, it):
    from .metrics import fov_scores_host
    gt, frame = it['HR_UW'], frame.contiguous()
    if frame.shape != gt.shape:
        raise RuntimeError('--eval_mode %s: result %s and ground truth %s differ in shape' % (run.config.EVAL.eval_mode, tuple(frame.shape), tuple(gt.shape)))
    return fov_scores_host(frame, gt)


def _device_scores(run, outs, items, vis=None):
    """--metrics device (extension, default 'host'): the scores of a network call's frames from ONE refvsr_score_frames launch (FOV: one
    refvsr_score_regions launch) on the caller's current stream -- which already waits for the results, pipelined mode included:
    INTEGRATION.md -- crossing to the host as 16 bytes per frame (FOV: 7 rectangles x 16); the frame itself is only copied when an
    image is written."""
    from . import ops
    from .metrics import fov_rects, fov_table, psnr_from_mse
    gts = [it['HR_UW'].to(run.dev) for it in items]              # (decoded bytes, channels-last: a quarter of the float frame)
    # flag_HD_in: the result is `scale` times the ground truth and the scores are those of its bicubic down-scale, which the
    # kernel forms while it stages its tiles (refvsr_score_frames_down): the big frame is read once where it lies
    down = int(run.config.scale) if run.config.flag_HD_in else 1     # (no FOV mode here: evaluate() refuses it for these configs)
    for o, g in zip(outs, gts):
        if tuple(o[0].shape) != (3, down * g.shape[-2], down * g.shape[-1]):
            raise RuntimeError('--metrics device: result %s and ground truth %s differ in shape' % (tuple(o[0].shape), tuple(g.shape)))
    if run.mode is FOV:
        h, w = gts[0].shape[-2:]
        sums = ops.score_regions([o[0] for o in outs], gts, fov_rects(h, w)).cpu().numpy()
        return [(fov_table(sm, h, w), {}) for sm in sums]
    sc = ops.score_frames([o[0] for o in outs], gts, win=7, **({'down': down} if down != 1 else {})).cpu().tolist()
    return [(np.array([psnr_from_mse(m), s]), {}) for m, s in sc]


def _colour(run, outs, items, vis):
    """The windows' 'eval_vis' dicts -> per window its images on the host, in the place of its scores: ONE conf_colormap launch."""
    from . import ops
    imgs = [x.cpu() for x in ops.conf_colormap([v[src] for v in vis for _, src in CONF_MAP_DIRS])]
    k = len(CONF_MAP_DIRS)
    return [(np.zeros(0), dict((CONF_MAP_DIRS[j][0], imgs[b * k + j]) for j in range(k))) for b in range(len(vis))]


# What the three modes differ in -- host: a frame's score when no launch of the call gave it; writes: whether the input / result (/ map)
# images are written; summary: the text of a clip's MEAN and the run's TOTAL; total: the run's v; end: what the score file gets after a summary
Mode = collections.namedtuple('Mode', 'host writes summary total end')
QUAL = Mode(_host_scores, lambda run: not run.quantitative_only, _line_summary,
            lambda res, n: np.array([sum(res['psnr']) / n, sum(res['ssim']) / n]), '\n')
FOV = Mode(_host_fov, lambda run: False, _fov_summary, lambda res, n: sum(res['fov']) / n if res['fov'] else np.zeros((6, 3, 2)), '')
CONF = Mode(None, lambda run: True, _line_summary, lambda res, n: np.zeros(0), '\n')


def _host_frame(out):
    """A result [1,3,h,w] on the host -> (what write_frame takes: 'uint8' results stay bytes, the float frame the host scores take).
    (result_dtype 'uint8' / 'float16', extensions: the scores are then those of the quantised frame; the PNG bytes are the same.)"""
    raw = out[0].cpu()
    frame = raw.float()
    return (raw, frame / 255.0) if raw.dtype == torch.uint8 else (frame, frame)


class _Run(object):
    """One evaluate() call: its options, each read once; the clip's sums; the video writer; the result dict."""

    def __init__(self, config, net, log, mode):
        E = config.EVAL
        self.config, self.net, self.log, self.mode, self.data = config, net, log, mode, E.data
        self.qualitative_only = bool(getattr(E, 'qualitative_only', False))
        self.quantitative_only = bool(getattr(E, 'quantitative_only', False))
        self.writes, self.video, self.use_ids = mode.writes(self), getattr(E, 'video_out', None), getattr(E, 'use_frame_ids', True)
        # --frame_group G (extension, default 1 = the reference's loop): G consecutive windows of a clip per network call
        # (SRNet.forward_group: the backward branches of the G frames as multi-map launches; results bit-identical); the per-frame time in
        # the score lines is then the group's time / G
        self.G = max(1, int(getattr(E, 'frame_group', 1) or 1))
        self.ckpt_name = os.path.basename(E.ckpt_abs_name) if E.ckpt_abs_name else 'seeded'
        root = os.path.join(E.LOG_DIR.save, E.eval_mode, self.ckpt_name.split('.')[0])
        self.out_root = os.path.join(root, E.data, datetime.datetime.now().strftime('%Y_%m_%d_%H%M'))
        os.makedirs(root, exist_ok=True)
        self.score_path = os.path.join(root, 'score_%s_%s.txt' % (E.data, E.eval_mode))
        self.ds = ClipSet(config)
        self.dev = next(net.parameters()).device
        # what scores (or colours) all frames of a network call in one launch; None: every frame is scored on the host
        on_device = getattr(E, 'metrics', 'host') == 'device' and not self.qualitative_only
        self.launch = _colour if mode is CONF else _device_scores if on_device else None
        # (the state to restore is the net's own: a caller's net may have been switched on without config.pipelined saying so)
        engines = getattr(net.Network, '_engines', None)
        self.was_pipelined = bool(engines[0].pipelined) if engines else bool(getattr(config, 'pipelined', False))
        self.res = {'psnr': [], 'ssim': [], 'seconds': [], 'frames': 0}
        if mode is FOV:
            self.res['fov'] = []
        self.said, self.writer, self.writer_clip, self.prev = False, None, None, None
        self.clip_v, self.clip_t, self.clip_n = 0.0, 0.0, 0

    def say(self, text, end='\n'):
        """log + score file: the run's first write starts the file."""
        self.log(text)
        with open(self.score_path, 'a' if self.said else 'w') as fh:
            fh.write(text + end)
        self.said = True

    def write_video(self, it, y):
        """--video_out y4m (extension): the frame's 'yuv' [1, 3sh/2, sw] -- 1.5 samples per pixel cross to the host -- appended to
        <out_root>/y4m/<clip>.y4m, one file per clip."""
        from .yuv import Y4MWriter
        a = y[0].cpu().numpy()
        if self.writer_clip != it['video_name']:
            self.close_video()
            path = os.path.join(self.out_root, 'y4m', '%s.y4m' % it['video_name'])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            self.writer = Y4MWriter(path, a.shape[0] * 2 // 3, a.shape[1], self.config.result_yuv, getattr(self.config.EVAL, 'video_fps', None) or (30, 1),
                                    getattr(self.config, 'yuv_range', None) or 'limited')
            self.writer_clip = it['video_name']
            self.res.setdefault('videos', []).append(path)
        self.writer.write(a)

    def close_video(self):
        if self.writer is not None:
            self.writer.close()
        self.writer = self.writer_clip = None

    def emit(self, it, out, lr_c, dt, score, yuv):
        """One frame of a call: its video frame, its score (the host's unless the call's launch gave it), its line, its images, the sums."""
        if self.video:
            self.write_video(it, yuv)
        if score is None or self.writes:                 # (else nothing reads the frame: it stays on the device)
            img, frame = _host_frame(out)
        v, maps = score if score is not None else (self.mode.host(self, frame, it), {})
        self.say('[EVAL {}|{}|{}][{}/{}][{}/{}] {} {}({:.5f}sec)'.format(
            self.config.mode, self.data, it['video_name'], it['video_idx'] + 1, it['video_len'], it['frame_idx'] + 1, it['frame_len'],
            it['frame_name'], _scores_tail(v), dt))
        if self.writes:
            name = os.path.join(it['video_name'], it['frame_name'].split('.')[0])
            for fmt in ('png', 'jpg'):
                for folder, im in [('input', lr_c), ('output', img)] + [(f, m.permute(2, 0, 1)) for f, m in maps.items()]:
                    write_frame(os.path.join(self.out_root, fmt, folder, '%s.%s' % (name, fmt)), im)
        self.clip_v, self.clip_t, self.clip_n, self.prev = self.clip_v + v, self.clip_t + dt, self.clip_n + 1, it
        if v.size:
            self.res['psnr'].append(float(v.flat[0]))
            self.res['ssim'].append(float(v.flat[1]))
        if self.mode is FOV:
            self.res['fov'].append(v)
        self.res['seconds'].append(dt)
        self.res['frames'] += 1

    def call(self, items, group=False, first=False):
        """One network call for the windows `items` and what follows it.  The two entries are the reference's own net(window) and
        forward_group; conf_map: the first is called with is_log=True and returns 'eval_vis', the second with want_conf=True.  Timed: from
        before the inputs' copy to the device to after the synchronize; scoring, colouring and writing are not."""
        t0 = time.time()
        if group:
            lrs, rfs = (stack_frames([it[k] for it in items]).to(self.dev) for k in ('LR_UW', 'LR_REF_W'))
            if lrs.dtype != torch.uint8:
                lrs, rfs = lrs.float().contiguous(), rfs.float().contiguous()
            got = self.net.forward_group(lrs, rfs, [it['frame_ids'] for it in items], is_first_frame=first, **({'want_conf': True} if self.mode is CONF else {}))
            outs, vis, yuv = got['result'], got['eval_vis'] if self.mode is CONF else None, got.get('yuv')
        else:
            it, = items
            lrs, rfs = it['LR_UW'][None].to(self.dev), it['LR_REF_W'][None].to(self.dev)
            kw = {'frame_ids': it['frame_ids']} if self.use_ids and 'frame_ids' in it else {}
            got = self.net(lrs, rfs, it['is_first'], is_log=self.mode is CONF, is_train=False, **kw)
            outs, vis, yuv = [got['result']], [got['eval_vis']] if self.mode is CONF else None, [got.get('yuv')]
        torch.cuda.synchronize()
        dt = (time.time() - t0) / len(items)
        scores = self.launch(self, outs, items, vis) if self.launch else [None] * len(items)
        for b, it in enumerate(items):
            self.emit(it, outs[b], lrs[b, lrs.shape[1] // 2], dt, scores[b], yuv[b] if self.video else None)

    def clip_summary(self):
        """The clip's MEAN line / block, named for the clip it summarises; resets the clip's sums."""
        if self.clip_n:
            head = '[MEAN EVAL {}|{}|{}][{}/{}]'.format(self.config.mode, self.data, self.prev['video_name'], self.prev['video_idx'], self.prev['video_len'])
            self.say(self.mode.summary(head, self.clip_v / self.clip_n, self.clip_t / self.clip_n, False), self.mode.end)
        self.clip_v, self.clip_t, self.clip_n = 0.0, 0.0, 0

    def total(self):
        n = max(self.res['frames'], 1)
        head = '[TOTAL {}|{}]'.format(self.ckpt_name, self.data)
        self.say(self.mode.summary(head, self.mode.total(self.res, n), sum(self.res['seconds']) / n, True), self.mode.end)

    def loop(self):
        """The per-frame loop (eval_qual_quan.py:39-128, eval_quan_FOV.py:55-232, eval_quan_conf_map.py:32-174).  In a grouped run the
        frames after a clip's first wait for a full group; the first goes alone through net(window) -- conf_map: through a forward_group
        of its one window, so that every call of the run returns its maps the same way."""
        pending = []

        def flush():
            if pending:
                self.call(pending, group=True)
                del pending[:]
        for i in range(len(self.ds)):
            it = self.ds[i]
            if it.get('is_continue'):
                continue
            if it['is_first']:
                flush()
                self.clip_summary()
                self.net.Network.reset()
            grouped = self.G > 1 and self.use_ids and 'frame_ids' in it
            if grouped and not it['is_first']:
                pending.append(it)
                if len(pending) == self.G:
                    flush()
            elif grouped and self.mode is CONF:
                self.call([it], group=True, first=True)
            else:
                self.call([it])
        flush()


def evaluate(config, net=None, log=print):
    """The reference's three evaluation loops as one; `--eval_mode` picks the per-mode entry (QUAL / FOV / CONF above).
    Returns dict(psnr=[..], ssim=[..], frames=N, seconds=[..], score_file, output_root).
    qual_quan (any other name): eval_qual_quan counterpart -- per frame PSNR / SSIM (--metrics host | device) and the input and result
    images (-quantitative_only: no images; -qualitative_only: no scores; --video_out y4m: also a video per clip, res['videos']).
    A name with FOV in it: eval_quan_FOV counterpart -- a frame's score is its FOV table (metrics.fov_table, [6 keys][fi, fo, fr][psnr, ssim]),
    whose key 1 fi pair is the per-frame line; the summaries are the reference's six-row blocks; no image is written (the reference has
    that part commented out); the tables are returned as res['fov'].
    A name with conf_map in it: eval_quan_conf_map counterpart -- no scores (psnr / ssim stay empty; --metrics, -qualitative_only and
    -quantitative_only have no effect, as in the reference's loop): per frame the input, the result and the four maps of 'eval_vis'
    coloured by ONE ops.conf_colormap launch per network call (CONF_MAP_DIRS names the folders); with --frame_group G > 1 the maps come
    from forward_group(want_conf=True).  RefVSR_IR has no such maps (the reference fails on None['conf_map'])."""
    E = config.EVAL
    mode = FOV if 'FOV' in str(E.eval_mode) else CONF if 'conf_map' in str(E.eval_mode) else QUAL
    video = getattr(E, 'video_out', None)
    if mode is CONF and config.network == 'RefVSR_IR':
        raise RuntimeError('--eval_mode %s: RefVSR_IR returns no confidence maps (config %s)' % (E.eval_mode, config.get('config')))
    if video and mode is not QUAL:
        raise RuntimeError(VIDEO_MODE_MESSAGE % E.eval_mode)
    if video and video != 'y4m':
        raise RuntimeError("--video_out: 'y4m' is the only container (got %r)" % (video,))
    if video and getattr(config, 'result_yuv', None) not in ('i420', 'i420p10'):
        raise RuntimeError("--video_out y4m needs config.result_yuv = 'i420' | 'i420p10' (Y4M frames are planar), got %r" % (getattr(config, 'result_yuv', None),))
    if mode is FOV and config.flag_HD_in:
        raise RuntimeError('--eval_mode %s: flag_HD_in configs are not supported (the reference scores a cv2.resize(INTER_CUBIC) of the result)' % E.eval_mode)
    if mode is CONF:
        config.save_sample = True            # eval_quan_conf_map.py:23: Network.forward(is_log=True) then returns 'eval_vis'
    if net is None:
        from . import SRNet
        if config.device != 'cuda':
            raise RuntimeError('refvsr_amd has no CPU path; run on the GPU (drop --cpu)')
        net = SRNet(config).to('cuda').eval()
        if E.ckpt_abs_name:
            log('Loading checkpoint %s: %s' % (E.ckpt_abs_name, load_checkpoint(net, E.ckpt_abs_name)))
    if mode is CONF:
        net.Network.config.save_sample = True            # (a caller's net may carry a config of its own)
    run = _Run(config, net, log, mode)
    if run.G > 1:
        net.Network.set_pipelined(True)          # (restored at the end: the caller's plain net(...) calls keep their stream contract)
    try:
        with torch.no_grad():
            run.loop()
    finally:
        run.close_video()
        if run.G > 1 and not run.was_pipelined:
            torch.cuda.synchronize()
            net.Network.set_pipelined(False)
    run.clip_summary()
    run.total()
    run.res['score_file'], run.res['output_root'] = run.score_path, run.out_root
    return run.res


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
