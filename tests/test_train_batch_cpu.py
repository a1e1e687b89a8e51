"""CPU: the definition of the training-batch formation (wave_mamba_amd/data.py, cpu_twin.paired_patches) against an independent
restatement written here from numpy primitives in the reference's order of operations (basicsr/data/paired_image_dataset.py:80-131
at scale 1: padding -> paired_random_crop -> random_augmentation -> img2tensor -> collate), the draw order, the host validation
and the C ABI's argument checks.  Everything after the division by 255 is a permutation, so every comparison is bit for bit."""
import random

import numpy as np
import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd import _lib, cpu_twin, data


def image_pair(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def augment(a, mode):
    """data_augmentation (transforms.py:223-268), as the reference spells it."""
    return [lambda x: x, np.flipud, np.rot90, lambda x: np.flipud(np.rot90(x)), lambda x: np.rot90(x, k=2),
            lambda x: np.flipud(np.rot90(x, k=2)), lambda x: np.rot90(x, k=3), lambda x: np.flipud(np.rot90(x, k=3))][mode](a)


def restated(pairs, rows, P, swap_rb=True):
    """The reference's order of operations, numpy primitives only."""
    out = ([], [])
    for index, top, left, mode in rows:
        for k, img in enumerate(pairs[index]):
            h, w = img.shape[:2]
            a = np.pad(img, ((0, max(0, P - h)), (0, max(0, P - w)), (0, 0)), mode="symmetric")     # cv2.BORDER_REFLECT
            a = a[top:top + P, left:left + P]
            a = augment(a, mode)
            if swap_rb:
                a = a[..., ::-1]
            out[k].append(a.transpose(2, 0, 1).astype(np.float32) / 255.)
    return tuple(torch.from_numpy(np.stack(o)) for o in out)


def assert_same(got, want, what):
    for name, g, w in zip(("lq", "gt"), got, want):
        assert g.dtype == torch.float32 and g.shape == w.shape, (what, name, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g, w), f"{what}: {name} differs in {int((g != w).sum())} elements"


def test_mode_table_is_the_reference_spelling():
    """The index table of the issue / the header against numpy's flipud / rot90 on a non-symmetric patch."""
    P = 5
    A = np.arange(P * P).reshape(P, P)
    i, j = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    table = [A[i, j], A[P - 1 - i, j], A[j, P - 1 - i], A[j, i], A[P - 1 - i, P - 1 - j], A[i, P - 1 - j], A[P - 1 - j, i],
             A[P - 1 - j, P - 1 - i]]
    for mode in range(8):
        assert np.array_equal(table[mode], augment(A, mode)), mode


def test_border_reflect_index_is_numpy_symmetric():
    for n, padded in [(7, 32), (20, 32), (9, 9), (1, 5), (50, 32)]:
        want = np.pad(np.arange(n), (0, max(0, padded - n)), mode="symmetric")[:padded]
        assert np.array_equal(cpu_twin.border_reflect_index(padded, n).numpy(), want), (n, padded)


@pytest.mark.parametrize("swap_rb", [True, False])
def test_all_modes_and_crop_extremes(swap_rb):
    P = 40
    pairs = [image_pair(97, 131, 1), image_pair(64, 200, 2), image_pair(41, 43, 3)]
    rows = []
    for index, (a, _) in enumerate(pairs):
        h, w = a.shape[:2]
        for mode in range(8):
            corners = [(0, 0), (h - P, w - P), (0, w - P), (h - P, 0), ((h - P) // 2, (w - P) // 3)]
            top, left = corners[(mode + index) % len(corners)]
            rows.append((index, top, left, mode))
        rows += [(index, 0, w - P, 2), (index, h - P, 0, 7), (index, h - P, w - P, 5)]
    assert_same(cpu_twin.paired_patches(pairs, rows, P, swap_rb), restated(pairs, rows, P, swap_rb), f"swap_rb={swap_rb}")


def test_images_smaller_than_the_patch():
    """Smaller in one dimension, in both, and by more than a factor of two (several reflections), across all modes."""
    P = 32
    pairs = [image_pair(20, 50, 4), image_pair(50, 20, 5), image_pair(20, 20, 6), image_pair(7, 9, 7)]
    rows = []
    for index, (a, _) in enumerate(pairs):
        h, w = a.shape[:2]
        for mode in range(8):
            rows.append((index, (max(h, P) - P) * (mode % 2), (max(w, P) - P) * ((mode // 2) % 2), mode))
    assert_same(cpu_twin.paired_patches(pairs, rows, P), restated(pairs, rows, P), "padding")


def test_host_store_and_batcher_form_the_twins_batch():
    pairs = [image_pair(45, 38, 8), image_pair(33, 70, 9)]
    store = data.DeviceImageStore("cpu")
    assert [store.add(*p) for p in pairs] == [0, 1] and len(store) == 2
    assert store.nbytes == 2 * 3 * (45 * 38 + 33 * 70)
    batcher = data.PairedPatchBatcher(store, gt_size=36, seed=5)
    rows = batcher.draw([1, 0, 1])
    assert_same(batcher.form(rows=rows), restated(pairs, rows, 36), "host batcher")
    out = (torch.zeros(3, 3, 36, 36), torch.zeros(3, 3, 36, 36))
    got = batcher.form(rows=rows, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert_same(out, restated(pairs, rows, 36), "host batcher, out=")


def test_draw_order_is_top_left_mode_per_sample():
    store = data.DeviceImageStore("cpu")
    shapes = [(97, 131), (64, 200), (20, 50), (41, 43)]
    for k, (h, w) in enumerate(shapes):
        store.add(*image_pair(h, w, 10 + k))
    P, seed, indices = 40, 1234, [3, 0, 2, 1, 0]
    rows = data.PairedPatchBatcher(store, gt_size=P, seed=seed).draw(indices)
    rng, want = random.Random(seed), []
    for index in indices:
        h, w = shapes[index]
        top = rng.randint(0, max(h, P) - P)
        left = rng.randint(0, max(w, P) - P)
        want.append((index, top, left, rng.randint(0, 7)))
    assert rows == want
    assert len({r[3] for r in rows}) > 1


def test_without_geometric_augs_no_mode_is_drawn():
    store = data.DeviceImageStore("cpu")
    store.add(*image_pair(97, 131, 20))
    P, seed = 40, 99
    rows = data.PairedPatchBatcher(store, gt_size=P, geometric_augs=False, seed=seed).draw([0] * 6)
    rng, want = random.Random(seed), []
    for _ in range(6):
        top = rng.randint(0, 97 - P)
        want.append((0, top, rng.randint(0, 131 - P), 0))             # two draws per sample: the stream is not advanced for a mode
    assert rows == want


def test_unequal_pair_shapes_raise():
    a, _ = image_pair(30, 40, 21)
    b, _ = image_pair(30, 41, 22)
    with pytest.raises(ValueError):
        data.DeviceImageStore("cpu").add(a, b)
    with pytest.raises(ValueError):
        cpu_twin.paired_patches([(a, b)], [(0, 0, 0, 0)], 16)
    with pytest.raises(ValueError):
        data.DeviceImageStore("cpu").add(a.astype(np.float32), a.astype(np.float32))


def test_scale_other_than_one_is_refused():
    store = data.DeviceImageStore("cpu")
    with pytest.raises(NotImplementedError, match="scale: 1"):
        data.PairedPatchBatcher(store, scale=2)
    with pytest.raises(NotImplementedError, match="scale: 1"):
        data.form_host_batch([], [], 16, "cuda:0", scale=4)


def test_out_of_range_rows_raise_before_anything_is_launched(monkeypatch):
    """Validation happens on the host before the table is touched: the library is made unloadable and the store is a host store,
    so reaching a launch (or a table) would fail differently."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libwavemamba_hip.so")
    store = data.DeviceImageStore("cpu")
    store.add(*image_pair(50, 60, 23))
    store.add(*image_pair(20, 60, 24))
    batcher = data.PairedPatchBatcher(store, gt_size=32, seed=0)
    bad = [(0, 19, 0, 0), (0, 0, 29, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, 8), (0, 0, 0, -1), (2, 0, 0, 0), (-1, 0, 0, 0),
           (1, 1, 0, 0), (0, 0, 0)]
    for row in bad:
        with pytest.raises(ValueError):
            batcher.form(rows=[(0, 18, 28, 7), row])
        with pytest.raises(ValueError):
            data.check_rows([row], store.shape, len(store), 32)
    with pytest.raises(ValueError):
        batcher.form()                                                 # neither indices nor rows
    with pytest.raises(ValueError):
        batcher.form(indices=[0], rows=[(0, 0, 0, 0)])
    with pytest.raises(ValueError):
        batcher.draw([2])
    assert data.check_rows([(0, 18, 28, 7), (1, 0, 28, 0)], store.shape, len(store), 32) == [(0, 18, 28, 7), (1, 0, 28, 0)]


def test_argument_validation_returns_before_launch():
    lib = _lib.load()
    fn = lib.wm_paired_patches_u8
    ptr = 0x7f0000000000                                               # never dereferenced: every call below returns before a launch
    assert fn(None, None, None, -1, 32, 1, None) == _lib.WM_EINVAL
    assert fn(ptr, ptr, ptr, 1, 0, 1, None) == _lib.WM_EINVAL
    assert fn(ptr, ptr, ptr, 1, -5, 1, None) == _lib.WM_EINVAL
    assert fn(None, None, None, 0, 32, 1, None) == _lib.WM_OK          # empty batch: a no-op, whatever the pointers
    assert fn(None, ptr, ptr, 1, 32, 1, None) == _lib.WM_ENULL
    assert fn(ptr, None, ptr, 1, 32, 1, None) == _lib.WM_ENULL
    assert fn(ptr, ptr, None, 1, 32, 1, None) == _lib.WM_ENULL
    assert fn(ptr + 4, ptr, ptr, 1, 32, 1, None) == _lib.WM_EALIGN
    assert fn(ptr, ptr + 2, ptr, 1, 32, 1, None) == _lib.WM_EALIGN
    # the grid limit: 2 B ceil(P / 32)^2 workgroups, at most 2^24 - 1
    assert fn(ptr, ptr, ptr, 1 << 23, 32, 1, None) == _lib.WM_EUNSUPPORTED
    assert fn(ptr, ptr, ptr, 1, 32 * 4096, 1, None) == _lib.WM_EUNSUPPORTED
    assert fn(ptr, ptr, ptr, 2, 2 ** 31 - 1, 1, None) == _lib.WM_EUNSUPPORTED


def test_operator_refuses_host_tables_and_wrong_tables():
    with pytest.raises(RuntimeError, match="CUDA"):
        wm.ops.paired_patches_u8(torch.zeros(2, 8, dtype=torch.int64), 32)
