"""Shared by tests/test_inference_batch_cpu.py and tests/test_inference_batch_gpu.py: the stub network, the reference's
data_augmentation in numpy, and the plan of the batched / self-ensembled pipeline spelled with cpu_twin's image I/O."""
import numpy as np
import torch

from wave_mamba_amd import cpu_twin

TINY = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)     # tests/test_inference_counterpart.py: CFG
INVERSE = {0: 0, 1: 1, 2: 6, 3: 3, 4: 4, 5: 5, 6: 2, 7: 7}
KEEP, TURN = (0, 1, 4, 5), (2, 3, 6, 7)


class StubNet(torch.nn.Module):
    """restoration_network returns its input: what comes out of the pipeline is then the I/O kernels' indexing alone."""

    def restoration_network(self, x):
        return x


def data_augmentation(image, mode):
    """basicsr/data/transforms.py:223-268 on a numpy (h, w, c) array: rot90 by mode // 2 quarter turns, then flipud for odd modes."""
    out = np.rot90(image, k=mode // 2) if mode // 2 else image
    return np.flipud(out) if mode % 2 else out


def images(shapes, seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]


def ensemble_plan(n_images):
    """(modes of the two pre launches per image, the post sources of image b in ascending mode order)."""
    where = {}
    for which, modes in enumerate((KEEP, TURN)):
        for b in range(n_images):
            for at, m in enumerate(modes):
                where[b, m] = (which, 4 * b + at, m)
    return [[where[b, m] for m in range(8)] for b in range(n_images)]


def ensemble_twin(forward, imgs, window, swap_rb):
    """The self-ensemble of equal-shaped uint8 images with cpu_twin's pre / post around `forward` ((N, 3, Hp, Wp) -> the same)."""
    xs = [cpu_twin.images_pre_u8([im for im in imgs for _ in modes], [m for _ in imgs for m in modes], window, swap_rb) for modes in (KEEP, TURN)]
    ys = [forward(x) for x in xs]
    h, w = imgs[0].shape[:2]
    return cpu_twin.images_post_u8(ys, [(h, w, srcs) for srcs in ensemble_plan(len(imgs))], swap_rb)
