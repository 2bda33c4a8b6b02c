"""The reference-side plug-in: the 3-line `models/archs/RefVSR_MI355X.py` INTEGRATION.md section 1 prints, resolved the way the
reference's shell resolves its arch -- `importlib.import_module('models.archs.' + config.network).Network(config)` under the shell's
`Network` attribute, models/SRNet.py:20-21, selected by `--network` (run.py:364,384) -- from an overlay directory that Python merges
into the (namespace) package `models.archs`.  The state dict of the shell is checked key by key, shape and dtype against the
reference shell's own (tests/golden/plugin_state_dict.json, written from the reference by tools/gen_golden.py --plugin-spec), and a
`module.`-prefixed checkpoint is loaded the way the reference's CKPT_Manager.load_ckpt loads it on a CPU run (ckpt_manager.py:50-56:
the wrapper's prefix dropped from every key, load_state_dict(strict=False)).  No GPU needed: construction, the state-dict contract and
checkpoint loading are host work."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = os.path.join(ROOT, 'tests', 'golden', 'plugin_state_dict.json')

CHILD = r'''
import importlib, json, os, re, sys, tempfile
ROOT, SPEC, name = sys.argv[1], sys.argv[2], sys.argv[3]
sys.dont_write_bytecode = True
doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
m = re.search(r"```python\n# models/archs/RefVSR_MI355X\.py[^\n]*\n(.*?)```", doc, re.S)
assert m, 'INTEGRATION.md section 1 no longer prints the plug-in file'
plugin = m.group(1)
assert len([l for l in plugin.strip().splitlines() if l.strip()]) <= 3
plugin = plugin.replace('/path/to/this/repo', ROOT)
if '_IR_' in name:             # INTEGRATION.md section 1: the RefVSR_IR family imports the same class from refvsr_amd.archs.RefVSR_IR
    assert 'refvsr_amd.model' in plugin
    plugin = plugin.replace('refvsr_amd.model', 'refvsr_amd.archs.RefVSR_IR')
over = tempfile.mkdtemp()
os.makedirs(os.path.join(over, 'models', 'archs'))
open(os.path.join(over, 'models', 'archs', 'RefVSR_MI355X.py'), 'w').write(plugin)
sys.path.insert(0, over)
network = 'RefVSR_MI355X'                                                           # run.py:384: config.network = args.network
arch = importlib.import_module('models.archs.' + network)                           # the shell's arch hook (puts the repo on sys.path)
import torch
cfg = importlib.import_module('refvsr_amd.configs.' + name).get_config('p', 'm', name)
cfg.cuda, cfg.device, cfg.dist = False, 'cpu', False
cfg.network = network
net = torch.nn.Module()
net.Network = arch.Network(cfg)
net.eval()
import refvsr_amd.model as mine
assert isinstance(net.Network, mine.Network), type(net.Network)
assert hasattr(net.Network, 'FlowNet')                                              # models/SRNet.py:44
want = json.load(open(SPEC))[name]                                                  # the reference shell's state dict
ks = net.state_dict()
assert [k for k, _, _ in want] == list(ks.keys()) or set(k for k, _, _ in want) == set(ks.keys()), set(k for k, _, _ in want) ^ set(ks.keys())
for k, shape, dtype in want:
    assert list(ks[k].shape) == shape and str(ks[k].dtype) == 'torch.' + dtype, (k, shape, dtype, ks[k].shape, ks[k].dtype)
# a released checkpoint = the DataParallel-wrapped shell's state dict: every key carries a leading `module.`
g = torch.Generator().manual_seed(5)
ck = {'module.' + k: torch.randn(shape, generator=g).to(getattr(torch, dtype)) for k, shape, dtype in want}
path = os.path.join(over, 'RefVSR_test.pytorch')
torch.save(ck, path)
res = net.load_state_dict({k[len('module.'):]: v for k, v in torch.load(path, map_location='cpu').items()}, strict=False)
assert not res.missing_keys and not res.unexpected_keys, (res.missing_keys[:3], res.unexpected_keys[:3])
for k, v in net.state_dict().items():
    assert torch.equal(v, ck['module.' + k]), k
# the call contract without a GPU: the build refuses CPU tensors loudly (no silent fallback), like any missing-extension case
x = torch.rand(1, 3, 3, 16, 16)
try:
    net.Network(x, x, True)
    raise SystemExit('a CPU call must raise')
except RuntimeError as e:
    assert 'GPU' in str(e) or 'librefvsr_hip' in str(e), e
print('PLUGIN_OK', name, len(ks))
'''


@pytest.mark.parametrize('name', ['config_RefVSR_small_L1', 'config_RefVSR_MFID_8K', 'config_RefVSR_IR_L1'])
def test_reference_shell_resolves_the_plugin_and_loads_a_module_prefixed_checkpoint(name):
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT, SPEC, name], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'PLUGIN_OK ' + name in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
