"""CPU side of the batched / graph-replayed / self-ensembled inference: the eight transforms against numpy's composition of the
reference's data_augmentation (transforms.py:223-268), the self-ensemble's indexing with a network that returns its input, the
float ensemble of inference.enhance against the explicit eight calls, the padding rule and the library's two new entry points."""
import numpy as np
import pytest
import torch

from oracle import oracle
from oracle import backend as oracle_backend
import wave_mamba_amd as wm
from wave_mamba_amd import _lib, cpu_twin

import inference_batch_cases as cases


@pytest.mark.parametrize("mode", range(8))
def test_dihedral_is_the_reference_s_data_augmentation(mode):
    a = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    t = torch.from_numpy(a)
    want = np.ascontiguousarray(cases.data_augmentation(a, mode))
    got = cpu_twin.dihedral(t, mode)
    assert got.shape == want.shape == ((7, 5, 3) if mode in cases.TURN else (5, 7, 3))
    assert np.array_equal(got.numpy(), want)
    assert torch.equal(cpu_twin.dihedral_inverse(got, mode), t)
    # the inverse is a mode of the same table, and the one the kernels' description states
    assert cpu_twin.DIHEDRAL_INVERSE[mode] == cases.INVERSE[mode]
    assert np.array_equal(cases.data_augmentation(want, cases.INVERSE[mode]), a)
    # on the last two axes of an (N, C, h, w) tensor, as inference.enhance uses it
    nchw = t.permute(2, 0, 1)[None]
    assert torch.equal(cpu_twin.dihedral(nchw, mode, (-2, -1))[0].permute(1, 2, 0), got)


@pytest.mark.parametrize("swap_rb", [True, False])
@pytest.mark.parametrize("h,w,window", [(1, 1, 1), (5, 7, 1), (33, 65, 32), (65, 33, 32)])
def test_self_ensemble_of_a_network_that_returns_its_input_is_the_input(h, w, window, swap_rb):
    """The mean of eight equal values b / 255 is b / 255 to a few units in the last place (the ascending sum rounds at 3 x, 5 x, ...),
    0.5 of a level away from any other: the uint8 result is the input exactly, and any wrong inverse, crop or pad origin shows
    (pads of 31 at window 32: the largest legal)."""
    imgs = cases.images([(h, w)] * 2, seed=h * 100 + w)
    out = cases.ensemble_twin(cases.StubNet().restoration_network, imgs, window, swap_rb)
    for im, o in zip(imgs, out):
        assert o.dtype == torch.uint8 and np.array_equal(o.numpy(), im)
    x = torch.from_numpy(imgs[0]).permute(2, 0, 1)[None].float() / 255.0
    if window == 1:                                                      # (enhance pads like check_image_size: no padding wanted here)
        assert torch.equal(wm.inference.to_uint8(wm.inference.enhance(cases.StubNet(), x, 1, ensemble=True)), wm.inference.to_uint8(x))


def test_images_pre_is_check_image_size_of_the_transformed_image():
    (im,) = cases.images([(33, 65)], seed=3)
    for mode in range(8):
        a = np.ascontiguousarray(cases.data_augmentation(im, mode))
        want = wm.inference.check_image_size(torch.from_numpy(a[:, :, ::-1].copy()).permute(2, 0, 1)[None].float() / 255.0, 32)
        got = cpu_twin.images_pre_u8([im], [mode], 32, swap_rb=True)
        assert got.shape == ((1, 3, 96, 64) if mode in cases.TURN else (1, 3, 64, 96))
        assert torch.equal(got, want)


def test_float_ensemble_is_the_explicit_eight_calls():
    """enhance(..., ensemble=True) with the tiny network on the oracle backend against rot90 / flip spelled out, bit for bit."""
    torch.manual_seed(0)
    net = wm.WaveMamba(**cases.TINY).eval()
    img = torch.rand(1, 3, 40, 56, generator=torch.Generator().manual_seed(77))
    prev = oracle_backend.set_ops_backend(oracle)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                             # sixteen forwards of maps this small: seconds each on many threads
    try:
        got = wm.inference.enhance(net, img, 32, ensemble=True)
        total = None
        for mode in range(8):
            x = torch.rot90(img, mode // 2, (-2, -1))
            x = (x.flip(-2) if mode % 2 else x).contiguous()
            y = wm.inference.enhance(net, x, 32)
            y = torch.rot90(y.flip(-2) if mode % 2 else y, -(mode // 2), (-2, -1))
            total = y if total is None else total + y
    finally:
        torch.set_num_threads(threads)
        oracle_backend.set_ops_backend(prev)
    assert got.shape == img.shape and not got.requires_grad
    assert torch.equal(got, total * 0.125)


def test_a_padding_that_reaches_the_image_size_raises():
    (im,) = cases.images([(3, 40)], seed=5)
    with pytest.raises(RuntimeError):
        cpu_twin.images_pre_u8([im], [0], 8)                             # 3 rows padded by 5
    with pytest.raises(RuntimeError):
        cpu_twin.images_pre_u8([im], [2], 8)                             # turned: 3 columns padded by 5
    assert cpu_twin.images_pre_u8([im[:, :8]], [0], 1).shape == (1, 3, 3, 8)
    with pytest.raises(RuntimeError):                                    # one launch, one padded shape
        cpu_twin.images_pre_u8([im[:, :16], im[:, :16]], [0, 2], 1)
    with pytest.raises(RuntimeError):                                    # F.pad's own refusal, through the float path
        wm.inference.enhance(cases.StubNet(), torch.rand(1, 3, 3, 40), 8, ensemble=True)


def test_the_tables_are_not_built_under_capture(monkeypatch):
    """Like grad_guard_table and adamw_table: the upload is a host-to-device copy."""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="a host-to-device copy must not be captured"):
        wm.ops.images_io_table(pre=[], post=[])


def test_library_exports_the_batched_image_entry_points():
    lib = _lib.load()
    assert lib.wm_abi_version() == _lib.ABI_VERSION == 34
    for name in ("wm_images_pre_u8", "wm_images_post_u8"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # argument checks that return before any launch: empty launches, NULL tables, the grid limits of the single-image kernels
    assert lib.wm_images_pre_u8(None, None, 0, 128, 128, 1, None) == _lib.WM_OK
    assert lib.wm_images_pre_u8(None, None, 1, 128, 128, 1, None) == _lib.WM_ENULL
    assert lib.wm_images_pre_u8(None, None, -1, 128, 128, 1, None) == _lib.WM_EINVAL
    assert lib.wm_images_pre_u8(8, 8, 65536, 128, 128, 1, None) == _lib.WM_EUNSUPPORTED
    assert lib.wm_images_pre_u8(8, 8, 1, 65536, 128, 1, None) == _lib.WM_EUNSUPPORTED
    assert lib.wm_images_pre_u8(4, 8, 1, 128, 128, 1, None) == _lib.WM_EALIGN
    assert lib.wm_images_post_u8(None, None, 0, 0, 0, None, 0, 0, 0, 0, 0, 0, 1, None) == _lib.WM_OK
    assert lib.wm_images_post_u8(None, None, 1, 8, 8, None, 0, 0, 0, 1, 8, 8, 1, None) == _lib.WM_ENULL
    assert lib.wm_images_post_u8(8, 8, 1, 8, 8, None, 1, 8, 8, 1, 8, 8, 1, None) == _lib.WM_ENULL      # a second tensor without memory
    assert lib.wm_images_post_u8(8, 8, 1, 8, 8, None, 0, 0, 0, 65536, 8, 8, 1, None) == _lib.WM_EUNSUPPORTED
    assert lib.wm_images_post_u8(8, 8, 1, 8, 8, None, 0, 0, 0, 1, 65536, 8, 1, None) == _lib.WM_EUNSUPPORTED
    assert lib.wm_images_post_u8(8, 8, 1, 8, 8, None, 0, 0, 0, -1, 8, 8, 1, None) == _lib.WM_EINVAL
