"""GPU side of the batched / graph-replayed / self-ensembled inference: wm_images_pre_u8 and wm_images_post_u8 against cpu_twin bit
for bit, the pipeline's indexing with a network that returns its input, and the tiny network of tests/test_inference_counterpart.py
eager against graphed, batched against single, ensembled against the twin's composition, scored, and across cache events."""
import copy

import numpy as np
import pytest
import torch

import wave_mamba_amd as wm
from wave_mamba_amd import cpu_twin

import inference_batch_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = wm.ops.IMAGES_IO_TILE
# (h, w, window): one pixel; smaller than a tile; pads of 31 at window 32, the largest legal, both ways round; and a shape that
# crosses the kernels' 32 x 32 LDS tile in both directions with a remainder (70 x 130)
SHAPES = [(1, 1, 1), (5, 7, 1), (33, 65, 32), (65, 33, 32), (2 * TILE + 6, 4 * TILE + 2, 8)]


def dev_images(imgs):
    return [torch.from_numpy(im).to(DEV) for im in imgs]


def outputs(n, Hp, Wp, seed):
    """fp32 'network outputs' with values below 0, above 1 and on exact halves of a level (v * 255 = k + 0.5 in float32)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(n, 3, Hp, Wp, generator=g) * 1.5 - 0.25
    half = (torch.randint(0, 255, y.shape, generator=g).float() + 0.5) / 255.0
    y = torch.where(torch.rand(y.shape, generator=g) < 0.25, half, y)
    return y


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("swap_rb", [True, False])
@pytest.mark.parametrize("h,w,window", SHAPES)
def test_images_pre_u8_is_the_twin_bit_for_bit(h, w, window, swap_rb, N):
    imgs = cases.images([(h, w)] * N, seed=h + w + N)
    dev = dev_images(imgs)
    for mode in range(8):
        table, none = wm.ops.images_io_table(pre=[(d, mode) for d in dev], window_size=window)
        assert none is None and table.n == N
        got = wm.ops.images_pre_u8(table, N, table.H, table.W, swap_rb)
        want = cpu_twin.images_pre_u8(imgs, [mode] * N, window, swap_rb)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), f"mode {mode}"
    for modes in (cases.KEEP, cases.TURN):                               # the ensemble's launches: one image, four modes, into `out`
        table, _ = wm.ops.images_io_table(pre=[(dev[0], m) for m in modes], window_size=window)
        out = torch.full((4, 3, table.H, table.W), -1.0, device=DEV)
        assert wm.ops.images_pre_u8(table, 4, table.H, table.W, swap_rb, out=out) is out
        assert torch.equal(out.cpu(), cpu_twin.images_pre_u8([imgs[0]] * 4, modes, window, swap_rb))


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("swap_rb", [True, False])
@pytest.mark.parametrize("h,w,window", SHAPES)
def test_images_post_u8_is_the_twin_bit_for_bit(h, w, window, swap_rb, N):
    pad = lambda n: n + (window - n % window) % window
    ys = [outputs(4 * N, pad(h), pad(w), 11 * h + w), outputs(4 * N, pad(w), pad(h), 13 * h + w)]
    assert int(((ys[0] * 255.0).frac() == 0.5).sum()) > 0                # the halves are there
    dev_ys = [y.to(DEV) for y in ys]

    def run(rows):
        dst = [torch.full((h, w, 3), 171, dtype=torch.uint8, device=DEV) for _ in rows]
        _, table = wm.ops.images_io_table(post=list(zip(dst, rows)))
        got = wm.ops.images_post_u8(table, dev_ys, swap_rb)
        want = cpu_twin.images_post_u8(ys, [(h, w, r) for r in rows], swap_rb)
        assert all(a is b for a, b in zip(got, dst))
        for n, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.cpu(), b), f"destination {n} of {rows}"

    for mode in range(8):                                                # k = 1: image n + 1 of the tensor that holds this mode's shape
        which = 1 if mode in cases.TURN else 0
        run([[(which, n + 1, mode)] for n in range(N)])
    run(cases.ensemble_plan(N))                                          # k = 8 over both tensors


@pytest.mark.parametrize("swap_rb", [True, False])
def test_one_source_of_mode_0_is_the_single_image_kernels(swap_rb):
    h, w = 2 * TILE + 6, 4 * TILE + 2
    (im,) = cases.images([(h, w)], seed=9)
    d = torch.from_numpy(im).to(DEV)
    table, _ = wm.ops.images_io_table(pre=[(d, 0)])
    x = wm.ops.images_pre_u8(table, 1, 128, 256, swap_rb)
    assert torch.equal(x, wm.ops.image_pre_u8(d, 128, swap_rb))
    y = outputs(1, 128, 256, 21).to(DEV)
    dst = torch.empty((h, w, 3), dtype=torch.uint8, device=DEV)
    _, table = wm.ops.images_io_table(post=[(dst, [(0, 0, 0)])])
    wm.ops.images_post_u8(table, y, swap_rb)
    assert torch.equal(dst, wm.ops.image_post_u8(y, h, w, swap_rb))


def test_the_operators_refuse_what_they_cannot_run():
    d = torch.zeros((3, 40, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="reaches the image's size"):
        wm.ops.images_io_table(pre=[(d, 0)], window_size=8)
    with pytest.raises(RuntimeError, match="reaches the image's size"):
        wm.ops.images_io_table(pre=[(d, 2)], window_size=8)
    with pytest.raises(RuntimeError, match="different shapes"):
        wm.ops.images_io_table(pre=[(d, 0), (d, 2)], window_size=1)
    with pytest.raises(RuntimeError, match="uint8"):
        wm.ops.images_io_table(pre=[(d.float(), 0)])
    with pytest.raises(RuntimeError, match="1 or 8 sources"):
        wm.ops.images_io_table(post=[(d, [(0, 0, 0), (0, 1, 1)])])
    table, post = wm.ops.images_io_table(pre=[(d, 0)], post=[(d, [(0, 1, 2)])], window_size=1)
    with pytest.raises(RuntimeError, match="the table holds"):
        wm.ops.images_pre_u8(table, 2, 3, 40)
    with pytest.raises(RuntimeError, match="out must be"):
        wm.ops.images_pre_u8(table, 1, 3, 40, out=torch.empty((1, 3, 3, 41), device=DEV))
    with pytest.raises(RuntimeError, match="the table reads 2 images of at least 40 x 3"):
        wm.ops.images_post_u8(post, torch.zeros((2, 3, 3, 40), device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        wm.ops.images_post_u8(post, torch.zeros((2, 3, 40, 3), device=DEV, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------------
# a network that returns its input through the pipeline: the kernels' indexing, the batching and the slots
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("ensemble", [False, True])
@pytest.mark.parametrize("batch", [1, 3])
def test_pipeline_of_a_network_that_returns_its_input(batch, ensemble, graphed):
    """Seven images of two shapes, A A A A B B A: at batch 3 a full batch, a batch cut short by a change of shape, one of two and one
    cut short by the end of the input; both slots and a plan used twice."""
    A, B = (40, 56), (33, 65)
    imgs = cases.images([A, A, A, A, B, B, A], seed=17)
    pipe = wm.inference.UInt8Pipeline(cases.StubNet(), DEV, window_size=32, batch=batch, ensemble=ensemble, graphed=graphed)
    out = list(pipe.run(imgs))
    assert len(out) == len(imgs)
    for n, (a, b) in enumerate(zip(out, imgs)):
        assert a.dtype == np.uint8 and np.array_equal(a, b), f"image {n}"
    if batch == 3:
        out = list(pipe.run(imgs[:4]))                                   # again, the plans (and graphs) kept
        assert all(np.array_equal(a, b) for a, b in zip(out, imgs))


# ------------------------------------------------------------------------------------------------------------------
# the tiny network
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    torch.manual_seed(0)
    return wm.WaveMamba(**cases.TINY).eval().to(DEV)


@pytest.fixture(scope="module")
def photos():
    """Five images of two shapes (padded to 128 x 128 and 128 x 256) and their eager single-image results."""
    return cases.images([(100, 120), (100, 120), (100, 120), (70, 150), (100, 120)], seed=4)


@pytest.fixture(scope="module")
def eager(net, photos):
    return list(wm.inference.UInt8Pipeline(net, DEV).run(photos))


def test_graphed_forward_and_graphed_pipeline_equal_the_eager_path(net, photos, eager):
    x = torch.rand(1, 3, 128, 256, generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        ref = net.restoration_network(x)
    fwd = wm.inference.GraphedForward(net)
    assert torch.equal(fwd(x), ref) and fwd.captures == 1
    pipe = wm.inference.UInt8Pipeline(net, DEV, graphed=True)
    for n, (a, b) in enumerate(zip(pipe.run(photos), eager, strict=True)):
        assert np.array_equal(a, b), f"image {n}"
    assert pipe.captures == 3                                            # the first shape in both slots, the second in one


def test_two_replays_with_eager_work_between_them_are_equal(net):
    g = torch.Generator().manual_seed(3)
    x, other = torch.rand(1, 3, 128, 128, generator=g).to(DEV), torch.rand(1, 3, 128, 256, generator=g).to(DEV)
    fwd = wm.inference.GraphedForward(net)
    first = fwd(x).clone()
    with torch.no_grad():
        net.restoration_network(other)                                   # same stream: its buffers come and go between the replays
        net.restoration_network(x[:, :, :, :128].contiguous())
    second = fwd(x)
    assert fwd.captures == 1 and torch.equal(first, second)


def test_batch_of_three_against_three_single_forwards(net, photos, eager, capsys):
    """The work split may depend on the batch: the float outputs to the project's bar (1e-4 relative per tensor, 0.03 of a level),
    the uint8 images to at most one level anywhere."""
    x = torch.rand(3, 3, 128, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        together = net.restoration_network(x)
        singles = torch.cat([net.restoration_network(x[i:i + 1].contiguous()) for i in range(3)])
    err = float((together - singles).norm() / singles.norm())
    assert err <= 1e-4, f"relative difference {err:.3e}"
    assert torch.equal(wm.inference.GraphedForward(net)(x), together)
    batched = list(wm.inference.UInt8Pipeline(net, DEV, batch=3).run(photos))
    differing = worst = count = 0
    for a, b in zip(batched, eager, strict=True):
        d = np.abs(a.astype(np.int16) - b.astype(np.int16))
        differing, worst, count = differing + int((d != 0).sum()), max(worst, int(d.max())), count + d.size
    with capsys.disabled():
        print(f"\n[inference batch] batch 3 against single forwards: float relative difference {err:.3e}; "
              f"{differing} of {count} uint8 values differ, by at most {worst}")
    assert worst <= 1


def test_float_ensemble_on_the_device_is_the_twin_s_composition(net):
    img = torch.rand(1, 3, 100, 120, generator=torch.Generator().manual_seed(6)).to(DEV)
    got = wm.inference.enhance(net, img, ensemble=True)
    total = None
    for mode in range(8):                                                # the same eight device forwards, composed on the host
        y = wm.inference.enhance(net, cpu_twin.dihedral(img, mode, (-2, -1)).contiguous()).cpu()
        y = cpu_twin.dihedral_inverse(y, mode, (-2, -1))
        total = y.clone() if total is None else total + y
    assert got.shape == img.shape and torch.equal(got.cpu(), total * 0.125)


@pytest.mark.parametrize("graphed", [False, True])
def test_ensemble_pipeline_is_the_twin_around_the_device_forwards(net, photos, graphed):
    """Two batch-4 forwards per image; cpu_twin's pre and post around the same forwards give the same uint8 image bit for bit."""
    def forward(x):
        with torch.no_grad():
            return net.restoration_network(x.to(DEV)).cpu()
    pipe = wm.inference.UInt8Pipeline(net, DEV, ensemble=True, graphed=graphed)
    some = photos[2:5]                                                   # two shapes
    for n, (a, im) in enumerate(zip(pipe.run(some), some, strict=True)):
        (want,) = cases.ensemble_twin(forward, [im], 128, True)
        assert np.array_equal(a, want.numpy()), f"image {n}"


def test_batched_graphed_run_scores_its_own_results(net, photos):
    targets = cases.images([p.shape[:2] for p in photos], seed=8)
    pipe = wm.inference.UInt8Pipeline(net, DEV, batch=2, graphed=True)
    plain = list(pipe.run(photos))
    scored = list(pipe.run(photos, targets))
    assert len(scored) == len(photos)
    for n, ((img, psnr, ssim), p, t) in enumerate(zip(scored, plain, targets)):
        assert np.array_equal(img, p), f"image {n}"
        want = wm.ops.psnr_ssim_y(torch.from_numpy(img).to(DEV), torch.from_numpy(t).to(DEV), 1, layout="HWC", bgr=True)[0].tolist()
        assert [psnr, ssim] == want, f"image {n}"
    res = wm.inference.evaluate(net, DEV, photos, targets, batch=2, graphed=True)
    assert res["psnr"] == [s[1] for s in scored] and res["ssim"] == [s[2] for s in scored]


def test_cache_of_one_shape_recaptures_and_stays_correct(net):
    g = torch.Generator().manual_seed(10)
    xs = [torch.rand(1, 3, 128, 128, generator=g).to(DEV), torch.rand(1, 3, 128, 256, generator=g).to(DEV)]
    with torch.no_grad():
        refs = [net.restoration_network(x) for x in xs]
    fwd = wm.inference.GraphedForward(net, max_shapes=1)
    for turn in range(4):
        assert torch.equal(fwd(xs[turn % 2]), refs[turn % 2]), f"call {turn}"
    assert fwd.captures == 4 and len(fwd._ent) == 1
    keep = wm.inference.GraphedForward(net, max_shapes=2)
    for turn in range(4):
        assert torch.equal(keep(xs[turn % 2]), refs[turn % 2])
    assert keep.captures == 2


def test_cold_weights_capture_whatever_streams_the_process_has_made(net):
    """torch hands streams out of a pool per device, round robin.  With the warm-up of a capture on a stream of its own, a stream
    that carried the handle of a side stream the forward reserves for captures produced the cold prepared weight copies, and the
    capture ended with hipErrorStreamCaptureUnjoined (inference._capture).  Here the pool stands right before such a handle.
    This relies on two things outside the project's surface: torch's stream pool handing the same handles out again (32 per device
    and priority, round robin, in torch 2.x up to the 2.10 this was written against) and the forward's registry of reserved side
    streams (wavemamba_arch._SIDE_STREAMS).  Should a torch release stop re-issuing handles, the handle is simply never met: the
    positioning is then skipped and the cold capture is still checked - nothing fails for a reason outside the project."""
    from wave_mamba_amd.archs import wavemamba_arch as arch
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(14)).to(DEV)
    with torch.no_grad():
        ref = net.restoration_network(x)                                 # the forward's side streams exist
    for reserved in arch._SIDE_STREAMS[(0, "capture")][::2]:
        before = prev = None
        for _ in range(200):                                             # once round the pool: which handle comes before the reserved one
            h = torch.cuda.Stream(DEV).cuda_stream
            if h == reserved.cuda_stream and prev is not None:
                before = prev
                break
            prev = h
        if before is not None:                                           # (None: this torch never re-issues the handle - no alias to provoke)
            any(torch.cuda.Stream(DEV).cuda_stream == before for _ in range(200))           # the next stream made is the reserved handle
        cold = copy.deepcopy(net)                                        # new parameters: nothing prepared
        assert torch.equal(wm.inference.GraphedForward(cold)(x), ref)


def test_a_weight_changed_in_place_is_not_served_from_a_stale_graph(net, photos):
    mine = copy.deepcopy(net)
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    fwd = wm.inference.GraphedForward(mine)
    pipe = wm.inference.UInt8Pipeline(mine, DEV, graphed=True)
    old = fwd(x).clone()
    old_img = list(pipe.run(photos[:1]))[0]
    with torch.no_grad():
        for p in mine.parameters():
            p.data.add_(0.02 * p.data.abs().mean())                      # through .data: no version moves
    wm.ops.conv2d_cache_clear()                                          # what such a writer must call (its docstring)
    with torch.no_grad():
        ref = mine.restoration_network(x)
    new = fwd(x)
    assert fwd.captures == 2 and torch.equal(new, ref) and not torch.equal(new, old)
    new_img = list(pipe.run(photos[:1]))[0]
    assert np.array_equal(new_img, list(wm.inference.UInt8Pipeline(mine, DEV).run(photos[:1]))[0])
    assert not np.array_equal(new_img, old_img)
    with torch.no_grad():
        next(mine.parameters()).mul_(1.5)                                # an in-place update autograd sees: the version moves
        ref = mine.restoration_network(x)
    assert torch.equal(fwd(x), ref) and fwd.captures == 3
