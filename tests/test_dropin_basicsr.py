"""Drop-in proof: the arch file works inside a `basicsr` package laid out like the reference's.

A temporary `basicsr/` package is assembled at test time: `utils/registry.py` is this repo's `wave_mamba_amd/registry.py`
(the surface of basicsr's Registry, uniqueness assertion included), `archs/__init__.py` is a stand-in written below with
what basicsr's does (import every `*_arch.py` of the folder as `basicsr.archs.<name>`, `build_network(opt)` pops 'type' and
instantiates from `ARCH_REGISTRY`), `utils/__init__.py` is empty, and THIS repo's `archs/wavemamba_arch.py` is copied into
`basicsr/archs/`.  Then exactly what the reference's callers do: the auto-scan, `build_network({'type': 'WaveMamba', ...})`,
`load_state_dict(torch.load(path)['params'], strict=False)` (inference_wavemamba.py:77), a forward.
"""
import importlib
import os
import shutil
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)

# basicsr/archs/__init__.py: the *_arch.py auto-scan and build_network
ARCHS_INIT = (
    "import importlib\n"
    "import os\n"
    "from basicsr.utils.registry import ARCH_REGISTRY\n"
    "_here = os.path.dirname(os.path.abspath(__file__))\n"
    "_arch_modules = [importlib.import_module('basicsr.archs.' + f[:-3])\n"
    "                 for f in sorted(os.listdir(_here)) if f.endswith('_arch.py')]\n"
    "def build_network(opt):\n"
    "    opt = dict(opt)\n"
    "    return ARCH_REGISTRY.get(opt.pop('type'))(**opt)\n")


@pytest.fixture()
def basicsr_tree(tmp_path):
    pkg = tmp_path / "basicsr"
    (pkg / "utils").mkdir(parents=True)
    (pkg / "archs").mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "utils" / "__init__.py").write_text("")
    shutil.copy(os.path.join(ROOT, "wave_mamba_amd", "registry.py"), pkg / "utils" / "registry.py")
    (pkg / "archs" / "__init__.py").write_text(ARCHS_INIT)
    shutil.copy(os.path.join(ROOT, "wave_mamba_amd", "archs", "wavemamba_arch.py"), pkg / "archs" / "wavemamba_arch.py")
    saved = {k: v for k, v in sys.modules.items() if k == "basicsr" or k.startswith("basicsr.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, str(tmp_path))
    importlib.invalidate_caches()
    try:
        yield tmp_path
    finally:
        sys.path.remove(str(tmp_path))
        for k in [k for k in sys.modules if k == "basicsr" or k.startswith("basicsr.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_arch_file_drops_into_basicsr(basicsr_tree, tmp_path):
    import wave_mamba_amd as wm                                   # the package is installed next to basicsr
    archs = importlib.import_module("basicsr.archs")              # runs the *_arch.py auto-scan
    reg = importlib.import_module("basicsr.utils.registry").ARCH_REGISTRY
    assert "WaveMamba" in reg.keys()
    dropped = sys.modules["basicsr.archs.wavemamba_arch"]
    assert reg.get("WaveMamba") is dropped.WaveMamba
    assert dropped.WaveMamba is not wm.WaveMamba                  # two module objects, two registries, no name clash
    assert dropped._hip_ops is wm.ops                             # operators come from the installed package

    torch.manual_seed(0)
    net = archs.build_network(dict(type="WaveMamba", **CFG))
    assert isinstance(net, torch.nn.Module) and hasattr(net, "restoration_network")
    for name in ("forward", "test", "test_tile", "check_image_size", "encode_and_decode", "print_network"):
        assert callable(getattr(net, name)), name

    # a reference-format checkpoint written by the package's trainer loads the way inference_wavemamba.py:77 does
    torch.manual_seed(1)
    donor = wm.WaveMamba(**CFG)
    ckpt = tmp_path / "net_g.pth"
    wm.trainer.save_network(donor, str(ckpt))
    net.load_state_dict(torch.load(str(ckpt), weights_only=True)["params"], strict=False)
    for (k1, v1), (k2, v2) in zip(net.state_dict().items(), donor.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2), k1

    # forward through the dropped-in module tree (CPU container: the oracle stands in for the HIP operators)
    from oracle import oracle
    x = torch.rand(1, 3, 32, 48, generator=torch.Generator().manual_seed(3))
    prev, dropped._OpsBackend.impl = dropped._OpsBackend.impl, oracle
    try:
        with torch.no_grad():
            y = net.eval().test(x)
    finally:
        dropped._OpsBackend.impl = prev
    from oracle import backend as oracle_backend
    with oracle_backend.ops_backend(oracle), torch.no_grad():
        y_pkg = donor.eval()(x)
    assert y.shape == x.shape and torch.equal(y, y_pkg)


def test_registering_twice_is_rejected_like_the_reference(basicsr_tree):
    importlib.import_module("basicsr.archs")
    reg = importlib.import_module("basicsr.utils.registry").ARCH_REGISTRY
    with pytest.raises(AssertionError):
        reg.register(sys.modules["basicsr.archs.wavemamba_arch"].WaveMamba)      # Registry._do_register's assertion
