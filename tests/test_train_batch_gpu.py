"""GPU: training batches formed on the device (ops.paired_patches_u8 / csrc/patch_batch.hip.h, wave_mamba_amd/data.py) against the
host statement of the reference's definition (cpu_twin.paired_patches, itself held to a numpy restatement by
tests/test_train_batch_cpu.py).  Everything after the division by 255 is a permutation: every comparison is torch.equal."""
import numpy as np
import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd import cpu_twin, data, trainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def image_pair(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def store_of(pairs):
    store = data.DeviceImageStore(DEV)
    for p in pairs:
        store.add(*p)
    return store


def assert_same(got, want, what):
    torch.cuda.synchronize()
    for name, g, w in zip(("lq", "gt"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype, tuple(g.shape))
        g = g.cpu()
        assert torch.equal(g, w), f"{what}: {name} differs in {int((g != w).sum())} of {g.numel()} elements"


def mode_sweep(pairs, P):
    """Every mode for every image, with crops at the extremes and in the interior."""
    rows = []
    for index, (a, _) in enumerate(pairs):
        h, w = a.shape[:2]
        dy, dx = max(h, P) - P, max(w, P) - P
        spots = [(0, 0), (dy, dx), (0, dx), (dy, 0), (dy // 2, dx // 3), ((2 * dy) // 3, dx // 2)]
        for mode in range(8):
            rows.append((index, *spots[(mode + index) % len(spots)], mode))
            rows.append((index, *spots[(mode + index + 3) % len(spots)], mode))
    return rows


@pytest.fixture(scope="module")
def main_case():
    """P = 40 (partial 32-tiles on both axes), images of different sizes and odd widths: neither the pitch nor the crop offset
    is 4-byte aligned.  The twin's batches, computed once."""
    P = 40
    pairs = [image_pair(97, 131, 1), image_pair(64, 200, 2), image_pair(41, 43, 3)]
    rows = mode_sweep(pairs, P)
    want = {swap: cpu_twin.paired_patches(pairs, rows, P, swap) for swap in (True, False)}
    return P, pairs, rows, want


@pytest.mark.parametrize("swap_rb", [True, False])
def test_parity_with_the_twin_all_modes_mixed_sizes(main_case, swap_rb):
    P, pairs, rows, want = main_case
    store = store_of(pairs)
    assert len(store) == 3 and store.nbytes == sum(2 * a.size for a, _ in pairs)
    batcher = data.PairedPatchBatcher(store, gt_size=P, swap_rb=swap_rb)
    got = batcher.form(rows=rows)
    assert got[0].shape == (len(rows), 3, P, P) and got[0].is_cuda
    assert_same(got, want[swap_rb], f"P=40 swap_rb={swap_rb}")


@pytest.mark.parametrize("P", [33, 32])
def test_small_patches_and_the_single_window(P):
    pairs = [image_pair(P, P, 10 + P), image_pair(P + 9, P + 2, 20 + P)]
    rows = mode_sweep(pairs, P)
    got = data.PairedPatchBatcher(store_of(pairs), gt_size=P).form(rows=rows)
    assert_same(got, cpu_twin.paired_patches(pairs, rows, P), f"P={P}")


def test_training_patch_size_from_a_wide_image():
    """The recipe's P = 512 (16 x 16 tiles per image) from an image as wide as a UHD one, odd pitch, one sample per mode class."""
    P = 512
    pairs = [image_pair(530, 3841, 60)]
    rows = [(0, 18, 3329, 0), (0, 0, 1001, 4), (0, 7, 0, 2), (0, 11, 2222, 7)]
    got = data.PairedPatchBatcher(store_of(pairs), gt_size=P).form(rows=rows)
    assert_same(got, cpu_twin.paired_patches(pairs, rows, P), "P=512")


def test_images_smaller_than_the_patch_are_reflected():
    """BORDER_REFLECT folded into the source index: smaller in one dimension, in both, and (7, 9) under P = 32 - several
    reflections - through every mode, the transposing ones included."""
    P = 32
    pairs = [image_pair(20, 50, 30), image_pair(50, 20, 31), image_pair(20, 20, 32), image_pair(7, 9, 33)]
    rows = mode_sweep(pairs, P)
    got = data.PairedPatchBatcher(store_of(pairs), gt_size=P).form(rows=rows)
    assert_same(got, cpu_twin.paired_patches(pairs, rows, P), "padding")


def test_kernel_clamps_a_wrong_table():
    """A raw table with top / left beyond their ranges (both ways) and mode 13, pointers valid: the kernel forms the clamped
    window with mode 13 & 7 - every output element comes from inside the image the row names."""
    P = 40
    pairs = [image_pair(97, 131, 40), image_pair(20, 50, 41)]
    store = store_of(pairs)
    raw = [(0, 10 ** 6, -3, 13), (0, -(10 ** 12), 10 ** 12, 13), (0, 58, 92, 13), (1, 5, 11, 13), (1, -1, 2 ** 40, 9)]
    clamped = [(0, 57, 0, 5), (0, 0, 91, 5), (0, 57, 91, 5), (1, 0, 10, 5), (1, 0, 10, 1)]
    table = torch.tensor([[store.pair(i)[0].data_ptr(), store.pair(i)[1].data_ptr(), *store.shape(i), top, left, mode, 0]
                          for i, top, left, mode in raw], dtype=torch.int64).to(DEV)
    got = wm.ops.paired_patches_u8(table, P)
    assert_same(got, cpu_twin.paired_patches(pairs, clamped, P), "clamped table")


def test_out_tensors(main_case):
    P, pairs, rows, want = main_case
    rows = rows[:7]
    batcher = data.PairedPatchBatcher(store_of(pairs), gt_size=P)
    B = len(rows)
    n = B * 3 * P * P
    arena = torch.full((2 * n + 5,), float("nan"), device=DEV)
    lq, gt = arena[1:1 + n].view(B, 3, P, P), arena[n + 3:2 * n + 3].view(B, 3, P, P)          # slices of a larger allocation
    got = batcher.form(rows=rows, out=(lq, gt))
    assert got[0].data_ptr() == lq.data_ptr() and got[1].data_ptr() == gt.data_ptr()
    assert_same((lq, gt), tuple(w[:B] for w in want[True]), "out=")
    assert bool(torch.isnan(arena[[0, n + 1, n + 2, 2 * n + 3, 2 * n + 4]]).all()), "wrote outside the out tensors"
    wide = torch.empty(B, 3, P, 2 * P, device=DEV)
    bad = [(wide[..., ::2], gt), (lq, wide[..., :P]), (lq[:-1], gt), (lq, gt.view(B, 3, P * P)), (lq.double(), gt), (lq.cpu(), gt),
           (lq, gt.permute(0, 1, 3, 2))]
    for out in bad:
        with pytest.raises(RuntimeError):
            batcher.form(rows=rows, out=out)


def test_host_path_equals_the_resident_store(main_case):
    P, pairs, rows, want = main_case
    got = data.form_host_batch(pairs, rows, P, DEV)
    assert_same(got, want[True], "form_host_batch")
    small = [image_pair(20, 50, 30), image_pair(50, 20, 31), image_pair(7, 9, 33)]
    rows32 = mode_sweep(small, 32)
    resident = data.PairedPatchBatcher(store_of(small), gt_size=32, swap_rb=False).form(rows=rows32)
    staged = data.form_host_batch(small, rows32, 32, DEV, swap_rb=False)
    torch.cuda.synchronize()
    assert torch.equal(staged[0], resident[0]) and torch.equal(staged[1], resident[1])
    assert_same(staged, cpu_twin.paired_patches(small, rows32, 32, False), "form_host_batch, padded")


def _eager_noise():
    """What a training loop does between two replays: kernels and allocations of its own."""
    for n, v in ((8, float("nan")), (320, 1e30), (65536, 1e30), (1 << 20, float("nan"))):
        t = torch.full((n,), v, device=DEV)
        del t
    torch.cuda.synchronize()


def test_captured_launch_sees_the_table_of_each_replay(main_case):
    """The launch alone on one stream in a graph (no parallel branches); the table is rewritten between replays, eager launches
    of the same kernel and other eager work run in between; each replay forms the rows current at that replay."""
    P, pairs, rows, want = main_case
    B = 6
    sets = [rows[0:B], rows[10:10 + B], rows[20:20 + B]]
    wants = [tuple(w[k:k + B] for w in want[True]) for k in (0, 10, 20)]
    batcher = data.PairedPatchBatcher(store_of(pairs), gt_size=P)
    batcher.update_table(rows=sets[0])
    lq, gt = torch.empty(B, 3, P, P, device=DEV), torch.empty(B, 3, P, P, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up off the capture's stream
        wm.ops.paired_patches_u8(batcher.table, P, out=(lq, gt))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wm.ops.paired_patches_u8(batcher.table, P, out=(lq, gt))
    table_ptr = batcher.table.data_ptr()
    other = data.PairedPatchBatcher(batcher.store, gt_size=P)
    for k in (0, 1, 2, 1, 0):
        batcher.update_table(rows=sets[k])
        assert batcher.table.data_ptr() == table_ptr
        lq.fill_(float("nan"))
        gt.fill_(float("nan"))
        graph.replay()
        assert_same((lq, gt), wants[k], f"replay with row set {k}")
        assert_same(other.form(rows=sets[(k + 1) % 3]), wants[(k + 1) % 3], "eager launch between replays")
        _eager_noise()
    graph.replay()                                              # no update: the table still holds set 0
    assert_same((lq, gt), wants[0], "replay without an update")


def test_train_step_on_a_formed_batch_equals_the_twins_batch():
    """train_step fed by batcher.form(rows=...) against train_step fed by the twin's batch moved to the device, from the same
    initial state (wf = 8 net, P = 64, B = 2): the inputs are bit-equal (asserted), so the loss dicts are equal, not close.

    Measured on MI355X.  The file alone in a process: the two dicts are equal ({'l_pix': 0.36992350220680237, 'l_freq':
    1.5313669443130493} both times).  After other GPU test files in the same process this assertion FAILS by one or two ulp of
    l_freq with l_pix equal and the inputs bit-equal: whole suite, twin 1.5313669443130493 / formed 1.5313671827316284; after
    test_ssim_loss_gpu.py + test_torch_library_ops.py, twin 1.5313670635223389 / formed 1.5313669443130493.  Cause, measured in
    such a process: 16 first steps from one state, twin-fed and kernel-fed alternating, give bit-equal forward outputs and
    bit-equal rfft2, but ops.l1_mean of ONE fixed (rfft2 out, rfft2 gt) pair returns 15.364481925964355 in 341 and
    15.364482879638672 in 59 of 400 calls.  wm_l1_mean_fwd adds its four workgroup sums with one fp32 atomic each, in completion
    order (csrc/loss.hip.h: "~1e-7 run to run"); a fixed-order sum needs a workspace the entry point does not have.  Nothing in the
    batch formation is involved.  The bound stays exact."""
    P = 64
    pairs = [image_pair(81, 97, 50), image_pair(70, 131, 51)]
    rows = [(0, 9, 20, 3), (1, 6, 67, 6)]
    cfg = dict(in_chn=3, wf=8, n_l_blocks=[1, 1, 1], n_h_blocks=[1, 1, 1], ffn_scale=2.0)

    def fresh():
        torch.manual_seed(0)
        net = wm.WaveMamba(**cfg).train().to(DEV)
        return net, trainer.make_optimizer(net)
    lq_t, gt_t = (t.to(DEV) for t in cpu_twin.paired_patches(pairs, rows, P))
    net, opt = fresh()
    want = trainer.train_step(net, opt, lq_t, gt_t)
    batcher = data.PairedPatchBatcher(store_of(pairs), gt_size=P)
    lq, gt = batcher.form(rows=rows)
    assert torch.equal(lq, lq_t) and torch.equal(gt, gt_t)
    net, opt = fresh()
    got = trainer.train_step(net, opt, lq, gt)
    print(f"twin batch {want}  formed batch {got}")
    assert set(got) == {"l_pix", "l_freq"} and got == want


def test_graphed_step_with_batcher_writes_the_steps_buffers():
    """trainer.graphed_step_with_batcher on a stand-in step object: the batch lands in step.lq / step.gt (no copy) and the step
    is then run on them."""
    P = 40
    pairs = [image_pair(97, 131, 1)]
    rows = [(0, 3, 5, 2), (0, 57, 91, 7)]

    class Step:
        def __init__(self):
            self.lq, self.gt = torch.zeros(2, 3, P, P, device=DEV), torch.zeros(2, 3, P, P, device=DEV)

        def __call__(self):
            return {"lq_sum": self.lq.double().sum(), "gt_sum": self.gt.double().sum()}
    step = Step()
    run = trainer.graphed_step_with_batcher(step, data.PairedPatchBatcher(store_of(pairs), gt_size=P))
    res = run(rows=rows)
    want = cpu_twin.paired_patches(pairs, rows, P)
    assert_same((step.lq, step.gt), want, "step buffers")
    assert float(res["lq_sum"]) == float(want[0].double().sum()) and float(res["gt_sum"]) == float(want[1].double().sum())
