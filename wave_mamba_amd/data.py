"""Training batches formed on the device: the counterpart of the TRAIN phase of the reference's PairedImageDataset.__getitem__
after the decode (basicsr/data/paired_image_dataset.py:80-131) and of the default collate that stacks its samples.

    padding              img_util.py:150-166     bottom / right to gt_size with cv2.BORDER_REFLECT
    paired_random_crop   transforms.py:24-83     top = randint(0, H - P), left = randint(0, W - P), one window for both images
    random_augmentation  transforms.py:270-275   mode = randint(0, 7): the eight flips / rotations of data_augmentation (:223-268)
    img2tensor           img_util.py:9-38        BGR -> RGB, HWC -> CHW, float32;  / 255 (imfrombytes(float32=True), :123-124)

The reference does this per sample on the CPU, on whole float32 images (99.5 MB each at UHD).  Here the uint8 images stay in
device memory (DeviceImageStore: 24.9 MB per UHD image), the host draws (top, left, mode) per sample - 64 bytes of table - and
one kernel (ops.paired_patches_u8, csrc/patch_batch.hip.h) writes the (B, 3, P, P) float32 `lq` / `gt` tensors that `feed_data`
would receive, bit for bit.  form_host_batch serves a set that does not fit in device memory: it stages only the crop windows.

scale == 1 only (the recipe's `scale: 1`, train_wavemamba_uhdll.yml); no decoding, no file or lmdb access, no mean / std.
cv2.BORDER_REFLECT is taken from OpenCV's documented definition (`fedcba|abcdefgh|hgfedcb`), which is numpy's 'symmetric'.

    store = DeviceImageStore("cuda:0")
    for lq, gt in decoded_pairs:                       # (h, w, 3) uint8, BGR as cv2 reads them
        store.add(lq, gt)
    batcher = PairedPatchBatcher(store, gt_size=512, seed=0)
    lq, gt = batcher.form(indices)                     # indices: the sampler's choice for this step
"""
import random

import numpy as np
import torch

_FIELDS = 8                  # int64 per table row: lq_ptr, gt_ptr, h, w, top, left, mode, reserved


def _check_scale(scale, who):
    if scale != 1:
        raise NotImplementedError(f"{who}: scale {scale!r} is not implemented - the recipe trains at `scale: 1` "
                                  "(lq and gt of one size, one crop window for both)")


def _as_u8_image(img, name):
    a = np.ascontiguousarray(img.cpu().numpy() if isinstance(img, torch.Tensor) else img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{name}: expected an (h, w, 3) uint8 image, got {a.shape} {a.dtype}")
    return a


def _check_pair_shapes(lq, gt):
    if lq.shape != gt.shape:                                       # transforms.py:54-57 (scale 1: one size)
        raise ValueError(f"Scale mismatches. GT ({gt.shape[0]}, {gt.shape[1]}) is not 1x multiplication of "
                         f"LQ ({lq.shape[0]}, {lq.shape[1]}).")


def check_rows(rows, shape_of, n_images, gt_size):
    """Host validation of (index, top, left, mode) rows: index names an image, the window lies inside the padded image, mode is
    0..7.  shape_of(index) -> (h, w).  Returns the rows as a list of int 4-tuples; ValueError otherwise."""
    P, checked = int(gt_size), []
    for row in rows:
        if len(row) != 4:
            raise ValueError(f"a row is (index, top, left, mode), got {tuple(row)!r}")
        index, top, left, mode = (int(v) for v in row)
        if not 0 <= index < n_images:
            raise ValueError(f"row {(index, top, left, mode)}: index outside 0..{n_images - 1}")
        h, w = shape_of(index)
        H, W = max(h, P), max(w, P)
        if not (0 <= top <= H - P and 0 <= left <= W - P):
            raise ValueError(f"row {(index, top, left, mode)}: the {P} x {P} window leaves the {h} x {w} image (padded to {H} x {W}): "
                             f"top in 0..{H - P}, left in 0..{W - P}")
        if not 0 <= mode <= 7:
            raise ValueError(f"row {(index, top, left, mode)}: mode outside 0..7")
        checked.append((index, top, left, mode))
    return checked


class DeviceImageStore:
    """uint8 image pairs resident on `device`, uploaded once.  add(lq, gt) -> the pair's index; len(store) pairs, store.nbytes
    bytes of images (whether a training set fits is the caller's arithmetic: 2 x 24.9 MB per UHD pair).  The tensors live as
    long as the store does, and a PairedPatchBatcher holds its store: a table never names freed memory.  With device 'cpu' the
    store keeps host tensors and the batcher forms its batches with cpu_twin.paired_patches."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._pairs = []

    def add(self, lq, gt):
        a, b = _as_u8_image(lq, "DeviceImageStore.add: lq"), _as_u8_image(gt, "DeviceImageStore.add: gt")
        _check_pair_shapes(a, b)
        self._pairs.append(tuple(torch.from_numpy(x.copy() if self.device.type == "cpu" else x).to(self.device) for x in (a, b)))
        return len(self._pairs) - 1

    def __len__(self):
        return len(self._pairs)

    @property
    def nbytes(self):
        return sum(t.numel() for pair in self._pairs for t in pair)

    def pair(self, index):
        """(lq, gt) uint8 tensors of pair `index` on the store's device."""
        return self._pairs[index]

    def shape(self, index):
        return tuple(self._pairs[index][0].shape[:2])


class PairedPatchBatcher:
    """Draws crops and augmentation modes like the reference's dataset and forms the batch from a DeviceImageStore.

    draw(indices) -> [(index, top, left, mode)]: per sample, from this object's own random.Random(seed), in the reference's order
    - top = randint(0, H - P), left = randint(0, W - P) (transforms.py:70-71), then mode = randint(0, 7) (transforms.py:271) only
    when geometric_augs is set (paired_image_dataset.py:114-115; mode 0 otherwise).  Seeded like the reference's process (its
    `random` module), it draws the reference's crops.
    form(indices=None, rows=None, out=None) -> (lq, gt), each (B, 3, P, P) float32: the rows drawn for `indices`, or the explicit
    `rows`, are validated on the host, written into a pinned table, copied to the persistent device table (non_blocking, current
    stream), and ops.paired_patches_u8 is launched on it - into `out=(lq, gt)` when given.
    update_table(indices=None, rows=None) does only the table update: a captured graph that holds the launch on `self.table`
    forms the new crops at its next replay.  (The table is re-allocated when the batch size changes; a graph is for one size.)

    The pinned table has two slots with an event each (the discipline of UInt8Pipeline's buffers): the host rewrites a slot only
    after the copy out of it has finished, so preparing step n + 1 does not wait for step n's copy.  The copy into the device
    table and the kernels that read it are ordered by the stream."""

    def __init__(self, store, gt_size=512, geometric_augs=True, seed=None, swap_rb=True, scale=1):
        _check_scale(scale, "PairedPatchBatcher")
        if int(gt_size) < 1:
            raise ValueError(f"PairedPatchBatcher: gt_size {gt_size!r}")
        self.store, self.gt_size, self.geometric_augs, self.swap_rb = store, int(gt_size), bool(geometric_augs), bool(swap_rb)
        self.rng = random.Random(seed)
        self.table = None                        # (B, 8) int64 on the store's device
        self._pin, self._copied, self._slot = [None, None], [None, None], 0

    def draw(self, indices):
        P, rows = self.gt_size, []
        for index in indices:
            index = int(index)
            if not 0 <= index < len(self.store):
                raise ValueError(f"PairedPatchBatcher.draw: index {index} outside 0..{len(self.store) - 1}")
            h, w = self.store.shape(index)
            top = self.rng.randint(0, max(h, P) - P)
            left = self.rng.randint(0, max(w, P) - P)
            mode = self.rng.randint(0, 7) if self.geometric_augs else 0
            rows.append((index, top, left, mode))
        return rows

    def _rows(self, indices, rows):
        if (indices is None) == (rows is None):
            raise ValueError("PairedPatchBatcher: give either indices (crops are drawn) or rows (index, top, left, mode)")
        if rows is None:
            rows = self.draw(indices)
        return check_rows(rows, self.store.shape, len(self.store), self.gt_size)

    def update_table(self, indices=None, rows=None):
        """Validate and write the rows into the device table (see the class).  Returns the rows written."""
        rows = self._rows(indices, rows)
        if self.store.device.type == "cpu":
            raise RuntimeError("PairedPatchBatcher.update_table: a host store has no device table (form() runs the host form)")
        B, dev = len(rows), self.store.device
        slot = self._slot
        self._slot ^= 1
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()                       # the last copy out of this pinned slot
        pin = self._pin[slot]
        if pin is None or pin.shape[0] != B:
            pin = self._pin[slot] = torch.empty((B, _FIELDS), dtype=torch.int64, pin_memory=True)
        host = pin.numpy()
        for k, (index, top, left, mode) in enumerate(rows):
            lq, gt = self.store.pair(index)
            host[k] = (lq.data_ptr(), gt.data_ptr(), lq.shape[0], lq.shape[1], top, left, mode, 0)
        if self.table is None or self.table.shape[0] != B:
            self.table = torch.empty((B, _FIELDS), dtype=torch.int64, device=dev)
        self.table.copy_(pin, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._copied[slot] = ev
        return rows

    def form(self, indices=None, rows=None, out=None):
        if self.store.device.type == "cpu":
            from . import cpu_twin
            lq, gt = cpu_twin.paired_patches(self.store._pairs, self._rows(indices, rows), self.gt_size, self.swap_rb)
            if out is None:
                return lq, gt
            out[0].copy_(lq)
            out[1].copy_(gt)
            return out[0], out[1]
        from . import ops
        self.update_table(indices, rows)
        return ops.paired_patches_u8(self.table, self.gt_size, self.swap_rb, out=out)


def form_host_batch(pairs, rows, gt_size, device, swap_rb=True, out=None, scale=1):
    """The same batch from HOST images, for a set that does not fit in device memory.  pairs: a sequence of (lq, gt) host images,
    (h, w, 3) uint8 of equal shape; rows: (index into pairs, top, left, mode) per sample.  Only each sample's crop window - the
    image's own rows / columns where it is smaller than gt_size - is copied into one pinned uint8 buffer (0.8 MB per image at
    gt_size 512, instead of the 99.5 MB float32 image the reference writes and re-reads), uploaded, and ops.paired_patches_u8
    runs on the staged windows with top = left = 0: the reflection of a short axis depends only on that axis' own length.
    -> (lq, gt) as PairedPatchBatcher.form, into `out` when given."""
    from . import ops
    _check_scale(scale, "form_host_batch")
    P, dev = int(gt_size), torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"form_host_batch: device {dev} is not a GPU (host batches: cpu_twin.paired_patches)")
    shapes = {}

    def shape_of(index):
        if index not in shapes:
            a, b = pairs[index]
            _check_pair_shapes(np.asarray(a), np.asarray(b))
            shapes[index] = tuple(np.asarray(a).shape[:2])
        return shapes[index]
    rows = check_rows(rows, shape_of, len(pairs), P)
    windows, total = [], 0
    for index, top, left, mode in rows:
        h, w = shape_of(index)
        ys = slice(top, top + P) if h >= P else slice(0, h)
        xs = slice(left, left + P) if w >= P else slice(0, w)
        hs, ws = min(h, P), min(w, P)
        windows.append((index, ys, xs, hs, ws, mode, total))
        total += 2 * hs * ws * 3
    pin = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
    pin_table = torch.empty((len(rows), _FIELDS), dtype=torch.int64, pin_memory=True)
    staged = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    host, host_table, base = pin.numpy(), pin_table.numpy(), staged.data_ptr()
    for k, (index, ys, xs, hs, ws, mode, at) in enumerate(windows):
        n = hs * ws * 3
        for which, img in enumerate(pairs[index]):
            a = _as_u8_image(img, "form_host_batch") if not isinstance(img, np.ndarray) else img
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"form_host_batch: expected (h, w, 3) uint8 images, got {a.shape} {a.dtype}")
            host[at + which * n: at + (which + 1) * n].reshape(hs, ws, 3)[...] = a[ys, xs]
        host_table[k] = (base + at, base + at + n, hs, ws, 0, 0, mode, 0)
    staged.copy_(pin, non_blocking=True)
    table = pin_table.to(dev, non_blocking=True)
    return ops.paired_patches_u8(table, P, swap_rb, out=out)
