"""What config.weight_precision = 'fp16' (the reference's fp16-autocast arithmetic) costs against the exact-fp32 reference: |dPSNR| =
|PSNR(build, GT) - PSNR(reference, GT)| per frame on the full-size fixtures of the mid_channels = 24 models (written by the imported
reference with fp32 weights), for both weight draws, next to the same figure of the default 'hi_lo' engine.  Reported, not a gate.

    python tools/weight_precision_parity.py            # one JSON line per (fixture, draw, mode); a table on stderr
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURES = [('e2e_full_S_270x480_t5', 'config_RefVSR_small_L1'), ('e2e_full_S_270x480_t5_long', 'config_RefVSR_small_MFID')]


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10.0 * np.log10(1.0 / max(mse, 1e-30))


def main():
    from refvsr_amd import SRNet, get_config, make_state_dict
    from refvsr_amd.synth import make_clip, window_indices
    dev = torch.device('cuda:0')
    for fx, name in FIXTURES:
        g = np.load(os.path.join(ROOT, 'tests', 'golden', fx + '.npz'))
        nfr, t = int(g['nframes']), 5
        lr, rf, gt = make_clip(nfr, 270, 480, seed=0)
        for variant in (None, 'plausible'):
            tag = 'p_' if variant else ''
            for mode in ('hi_lo', 'fp16'):
                cfg = get_config('p', 'm', name)
                cfg.frame_num, cfg.save_sample, cfg.weight_precision = t, False, mode
                net = SRNet(cfg).to(dev).eval()
                net.load_state_dict(make_state_dict(cfg, 1234, variant=variant))
                d = []
                for f in range(nfr):
                    w = window_indices(f, nfr, t)
                    res = net(lr[w][None].to(dev), rf[w][None].to(dev), f == 0)['result'].cpu()
                    d.append(abs(psnr(res, gt[f][None]) - float(g[tag + 'psnr_%d' % f])))
                rec = dict(tool='weight_precision_parity', fixture=fx, config=name, weights=variant or 'random', weight_precision=mode,
                           frames=nfr, dpsnr_max=float('%.3e' % max(d)), dpsnr_mean=float('%.3e' % (sum(d) / len(d))),
                           dpsnr=[float('%.2e' % v) for v in d])
                print(json.dumps(rec), flush=True)
                print('%-28s %-9s %-6s  max |dPSNR| %.3e dB  mean %.3e dB' % (fx, variant or 'random', mode, max(d), sum(d) / len(d)),
                      file=sys.stderr, flush=True)
                del net
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
