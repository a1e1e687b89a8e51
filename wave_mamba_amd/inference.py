"""Counterpart of the reference's inference caller for the hot path (inference_wavemamba.py:28-36, :99-113)
and of its image <-> tensor conventions (basicsr/utils/img_util.py:67-94) and PSNR
(comput_psnr_ssim.py:434-438), on tensors instead of image files (no cv2 / datasets in scope).  Its evaluation loop
(:116-135, Y-channel PSNR / SSIM on the device): UInt8Pipeline.run(images, targets) and evaluate().

    pad (reflect, to a multiple of 128)  ->  EnhanceNet.restoration_network(x) under no_grad
    ->  crop back to (h, w)  ->  clamp [0,1] * 255, round  ->  uint8  ->  PSNR against a target
"""
import torch
import torch.nn.functional as F


def check_image_size(x, window_size=128):
    """inference_wavemamba.py:28-36: reflect-pad bottom/right so H and W are multiples of window_size."""
    _, _, h, w = x.shape
    pad_h = (window_size - h % window_size) % window_size
    pad_w = (window_size - w % window_size) % window_size
    return F.pad(x, (0, pad_w, 0, pad_h), "reflect")


@torch.no_grad()
def enhance(net, img, window_size=128, ensemble=False):
    """img: (B, 3, h, w) float in [0, 1] on the model's device -> restored image, same shape
    (inference_wavemamba.py:99-113: pad -> restoration_network -> crop).
    ensemble=True: the geometric self-ensemble - the mean over the eight modes m of data_augmentation (transforms.py:223-268) of
    inverse_m(enhance(net, aug_m(img))), each transformed image padded after its transform; the sum runs in ascending mode order in
    the image's dtype and is multiplied by 1 / 8 (cpu_twin.dihedral, the order of ops.images_post_u8)."""
    if ensemble:
        from . import cpu_twin
        total = None
        for mode in range(8):
            turned = cpu_twin.dihedral(img, mode, (-2, -1)).contiguous()
            y = cpu_twin.dihedral_inverse(enhance(net, turned, window_size), mode, (-2, -1))
            total = y.clone() if total is None else total + y
        return total * 0.125
    _, _, h, w = img.shape
    out = net.restoration_network(check_image_size(img, window_size))
    return out[:, :, :h, :w]


def to_uint8(t):
    """tensor2img's quantisation (img_util.py:67-94, min_max=(0,1)): clamp, scale by 255, round."""
    return (t.detach().float().clamp(0, 1) * 255.0).round().to(torch.uint8)


def psnr_uint8(a, b):
    """20*log10(255/sqrt(mse)) on uint8-valued images (comput_psnr_ssim.py:434-438, crop_border 0, RGB)."""
    mse = (a.double() - b.double()).pow(2).mean()
    if float(mse) == 0.0:
        return float("inf")
    return float(20.0 * torch.log10(255.0 / mse.sqrt()))


# ------------------------------------------------------------------------------------------------------------------
# Captured forwards: below UHD the forward's kernels take less time than the host needs to launch them.
# ------------------------------------------------------------------------------------------------------------------
def _weights_signature(net):
    """What a captured forward of `net` depends on beyond its input: every parameter's and buffer's address and version, and the
    generation of the prepared weight copies (ops.conv2d_cache_clear: a write through `.data` bumps no version) - the rule of
    ops._PreparedCache."""
    from . import ops
    return (ops.prepared_generation(),) + tuple((t.data_ptr(), t._version) for t in list(net.parameters()) + list(net.buffers()))


def _capture(step, device):
    """Run `step` once eagerly (prepared-weight caches, allocator, the forward's side streams) and capture it into a graph ->
    (graph, step's result under capture).  The sequence of tests/test_gpu_parity.py::test_hip_graph_capture_after_a_multi_stream_forward
    and of bench.py's graph leg, with one difference from the latter: the warm-up runs on the CURRENT stream, not on a new side
    stream.  torch hands streams out of a pool of 32 per device, round robin, so a stream made here can carry the handle of one of
    the side streams the forward reserves for captures (wavemamba_arch._side_streams), and every new main stream makes the
    forward create three more.  A prepared weight copy that the warm-up produced on such a handle is then waited for, under
    capture, through an event of a stream that is itself capturing - and the capture ends with hipErrorStreamCaptureUnjoined
    (measured: cold caches and an aliased handle fail, warm caches or no alias pass).  On the current stream the
    copies come from the streams an eager forward of the caller would use.  Thread-local capture mode when a process group is
    initialised (its watchdog thread polls events while this thread captures)."""
    import gc
    import torch.distributed as dist
    with torch.cuda.device(device):
        step()
        graph = torch.cuda.CUDAGraph()
        mode = {"capture_error_mode": "thread_local"} if dist.is_available() and dist.is_initialized() else {}
        torch.cuda.synchronize(device)
        # No graph may be destroyed while this one is captured: ~CUDAGraph calls hipGraphDestroy, which a capturing stream refuses,
        # and the error leaves a destructor - the process aborts.  Graphs that are garbage go now, and the cycle collector, which
        # could find one in the middle of the capture (torch.cuda.graph does not collect on entry any more), rests until the end.
        gc.collect()
        resting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, **mode):
                out = step()
        finally:
            if resting:
                gc.enable()
    return graph, out


class GraphedForward:
    """net.restoration_network as captured graphs: one per input shape (N, Hp, Wp), with a static input and a static output.

        fwd = GraphedForward(net)
        y = fwd(x)            # x: (N, 3, Hp, Wp) float32 on the net's device, Hp and Wp multiples of the window (check_image_size)

    The first call with a shape runs one eager forward on the current stream and captures (_capture); later calls copy x into the static input and
    replay - bit-equal to the eager forward.  The result is the graph's static output: it is overwritten by the next call with
    that shape (clone it to keep it).  At most `max_shapes` graphs are kept, the least recently used leaving first - each owns a
    private memory pool, gigabytes at 3840 x 2160.  Every graph is dropped when a parameter or buffer of the net changes its
    address or version, or ops.conv2d_cache_clear has run (_weights_signature).  `captures` counts the captures made."""

    def __init__(self, net, max_shapes=4):
        import collections
        if int(max_shapes) < 1:
            raise ValueError(f"GraphedForward: max_shapes must be at least 1, got {max_shapes}")
        self.net, self.max_shapes, self.captures = net, int(max_shapes), 0
        self._ent = collections.OrderedDict()          # (device, N, Hp, Wp) -> (graph, static input, static output)
        self._sig = None

    def _drop(self, device, everything=False):
        torch.cuda.synchronize(device)                 # no graph is destroyed under its own replay
        if everything:
            self._ent.clear()
        else:
            self._ent.popitem(last=False)

    @torch.no_grad()
    def __call__(self, x):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3):
            raise RuntimeError("GraphedForward: expected a (N, 3, Hp, Wp) float32 CUDA tensor, got "
                               + (f"{tuple(x.shape)} {x.dtype} on {x.device}" if isinstance(x, torch.Tensor) else type(x).__name__))
        home = next((p.device for p in self.net.parameters()), x.device)
        if x.device != home:
            raise RuntimeError(f"GraphedForward: the input is on {x.device}, the network on {home}")
        sig = _weights_signature(self.net)
        if sig != self._sig:
            if self._ent:
                self._drop(x.device, everything=True)
            self._sig = sig
        key = (x.device, x.shape[0], x.shape[2], x.shape[3])
        ent = self._ent.get(key)
        if ent is None:
            while len(self._ent) >= self.max_shapes:
                self._drop(x.device)
            static_in = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            static_in.copy_(x)
            graph, out = _capture(lambda: self.net.restoration_network(static_in), x.device)
            self.captures += 1
            ent = self._ent[key] = (graph, static_in, out)
        else:
            self._ent.move_to_end(key)
            ent[1].copy_(x)
        ent[0].replay()
        return ent[2]


class _BatchPlan:
    """What the batched UInt8Pipeline owns per (image shape, batch, slot, scored): the pinned and device staging buffers, the static
    network inputs, the two device tables and - graphed - the captured pre -> forward -> post (-> psnr_ssim_y).  Everything a launch
    names is allocated here, before any capture, so a graph holds no pointer that moves."""

    _ENSEMBLE_MODES = ((0, 1, 4, 5), (2, 3, 6, 7))     # the shape-keeping transforms and the transposing ones: two batches

    def __init__(self, pipe, h, w, B, scored, crop_border):
        ops, dev = pipe.ops, pipe.device
        self.B, self.scored, self.crop = B, scored, crop_border          # (no reference to `pipe`: a cycle would leave the graph to the collector)
        shape = (B, h, w, 3)
        self.pin_in, self.pin_out = (torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(2))
        self.dev_in, self.res = (torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(2))
        self.pin_tgt = torch.empty(shape, dtype=torch.uint8, pin_memory=True) if scored else None
        self.dev_tgt = torch.empty(shape, dtype=torch.uint8, device=dev) if scored else None
        self.pin_met = torch.empty((B, 2), dtype=torch.float64, pin_memory=True) if scored else None
        mode_sets = self._ENSEMBLE_MODES if pipe.ensemble else ((0,),)
        self.pre, where = [], {}
        for which, modes in enumerate(mode_sets):
            table, _ = ops.images_io_table(pre=[(self.dev_in[b], m) for b in range(B) for m in modes], window_size=pipe.window)
            self.pre.append((table, torch.empty((table.n, 3, table.H, table.W), dtype=torch.float32, device=dev)))
            for b in range(B):
                for at, m in enumerate(modes):
                    where[b, m] = (which, len(modes) * b + at, m)
        modes = sorted(m for ms in mode_sets for m in ms)                      # the sum runs in ascending mode order
        _, self.post = ops.images_io_table(post=[(self.res[b], [where[b, m] for m in modes]) for b in range(B)])
        self.up_done = self.consumed = self.dl_done = None
        self.graph = self.met = self.signature = None

    def _step(self, pipe):
        ops = pipe.ops
        ys = [pipe.net.restoration_network(ops.images_pre_u8(t, t.n, t.H, t.W, pipe.swap_rb, out=x)) for t, x in self.pre]
        ops.images_post_u8(self.post, ys, pipe.swap_rb)
        if not self.scored:
            return None
        return ops.psnr_ssim_y(self.res, self.dev_tgt, self.crop, layout="HWC", bgr=pipe.swap_rb)

    def launch(self, pipe):
        """pre -> forward(s) -> post (-> metrics) on the current stream, eagerly or as one replay -> the (B, 2) metrics or None."""
        if not pipe.graphed:
            return self._step(pipe)
        sig = _weights_signature(pipe.net)
        if self.graph is None or sig != self.signature:
            if self.graph is not None:
                torch.cuda.synchronize(pipe.device)
                self.graph = self.met = None
            self.graph, self.met = _capture(lambda: self._step(pipe), pipe.device)
            self.signature = sig
            pipe.captures += 1
        self.graph.replay()
        return self.met


# ------------------------------------------------------------------------------------------------------------------
# uint8 host images in, uint8 host images out (inference_wavemamba.py:99-113 end to end):
# pinned double-buffered H2D / D2H on side streams under the previous / next image's forward.
# ------------------------------------------------------------------------------------------------------------------
class UInt8Pipeline:
    """enhance host uint8 images (h, w, 3; BGR as cv2 reads them, or RGB with swap_rb=False) with the network on `device`.

    Per image: pinned staging buffer -> H2D on the upload stream -> wm_image_pre_u8 (CHW, / 255, reflect pad) ->
    restoration_network -> wm_image_post_u8 (crop, clamp, * 255, round, HWC) -> D2H on the download stream into a pinned
    buffer.  Two buffers each way, events between the streams: the copies of images i + 1 / i - 1 run under the forward
    of image i.  `run(images)` yields numpy uint8 results in order.

    `run(images, targets)` also scores every result against its ground truth (host uint8, same shape) on the device, as the
    reference's evaluation loop does (inference_wavemamba.py:116-117: Y-channel PSNR / SSIM, crop_border 1): the target travels
    with its input on the upload stream, ops.psnr_ssim_y reads the device result before the download, and the two doubles come
    back with the image's copy.  It then yields (image, psnr, ssim).

    Three opt-in switches, for images below UHD, where the forward's kernels take less time than the host needs to launch them
    (profiles/inference_pipeline/README.md); with none given every call launches what is described above:
      batch > 1      consecutive images of equal shape are enhanced in one forward (wm_images_pre_u8 / wm_images_post_u8, N images
                     per launch); a change of shape or the end of the input flushes a short batch;
      ensemble=True  geometric self-ensemble: per image the eight transforms of data_augmentation as two forwards of four (the
                     shape-keeping modes 0, 1, 4, 5 and the transposing 2, 3, 6, 7; of 4 * batch with batch > 1), turned back and
                     averaged in fp32 in ascending mode order before the quantisation;
      graphed=True   pre -> forward -> post (-> psnr_ssim_y) replay from a captured graph per (image shape, batch, slot); a graph is
                     dropped when a weight changes (GraphedForward's rule).  `captures` counts the captures made.
    In these modes a step's buffers and device tables live in a _BatchPlan per (shape, batch, slot) - at most `max_plans`, the least
    recently used leaving first; the two slots, the two side streams and their events work as above.  Graphed, every plan owns
    its graph and the graph its private memory pool - a whole forward's intermediates, gigabytes at 3840 x 2160 - so one image shape
    costs two such pools (one per slot), a short last batch two more: lower `max_plans` (at least 2) where memory is short."""

    def __init__(self, net, device, window_size=128, swap_rb=True, batch=1, ensemble=False, graphed=False, max_plans=8):
        from . import ops
        import collections
        if int(batch) < 1 or int(max_plans) < 2:
            raise ValueError(f"UInt8Pipeline: batch must be at least 1 and max_plans at least 2, got {batch} and {max_plans}")
        self.net, self.device, self.window, self.swap_rb, self.ops = net, torch.device(device), window_size, swap_rb, ops
        self.batch, self.ensemble, self.graphed, self.max_plans, self.captures = int(batch), bool(ensemble), bool(graphed), int(max_plans), 0
        self._plans = collections.OrderedDict()         # (h, w, B, slot, scored, crop_border) -> _BatchPlan
        self.up, self.down = torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)
        self._pin_in, self._pin_out, self._dev_in = [None, None], [None, None], [None, None]
        self._pin_tgt, self._dev_tgt, self._pin_met = [None, None], [None, None], [None, None]   # run(images, targets) only
        self._up_done = [None, None]       # per slot: the last H2D copy out of pin_in[slot] (the host may then refill it)
        self._consumed = [None, None]      # per slot: main-stream event after image_pre_u8 has read dev_in[slot]
                                           # (with targets: after psnr_ssim_y has read dev_tgt[slot])

    def _buf(self, store, slot, shape, pinned, dtype=torch.uint8):
        t = store[slot]
        if t is None or tuple(t.shape) != tuple(shape):
            t = (torch.empty(shape, dtype=dtype, pin_memory=True) if pinned
                 else torch.empty(shape, dtype=dtype, device=self.device))
            store[slot] = t
        return t

    @torch.no_grad()
    def run(self, images, targets=None, crop_border=1):
        import numpy as np
        if self.batch > 1 or self.ensemble or self.graphed:
            yield from self._run_batched(images, targets, crop_border)
            return
        main = torch.cuda.current_stream(self.device)
        pending = []                                   # (pinned output, pinned metrics or None, download-done event)
        uploaded = None
        it = iter(images) if targets is None else zip(images, targets, strict=True)

        def upload(item, slot):
            """Stage the image (and its target) of `item` into slot: host -> pinned -> device on the upload stream.
            Returns ((device image, device target or None), event).  Orderings (all cross-stream):
              * the host refills pin_in[slot] (pin_tgt[slot]) only after the previous H2D copies out of it have finished;
              * the H2D copies into dev_in[slot] (dev_tgt[slot]) wait for main's image_pre_u8 (psnr_ssim_y) of the previous
                image of this slot;
              * the device buffer is allocated with `up` current (its pool), waits for main when it is (re)allocated -
                a fresh block may be memory that kernels still queued on main are using - and is recorded on main,
                which reads it."""
            img, tgt = (item, None) if targets is None else item
            if tgt is not None and tuple(np.shape(tgt)) != tuple(np.shape(img)):
                raise ValueError(f"UInt8Pipeline.run: target shape {tuple(np.shape(tgt))} != image shape {tuple(np.shape(img))}")
            a = torch.from_numpy(np.ascontiguousarray(img))
            t = None if tgt is None else torch.from_numpy(np.ascontiguousarray(tgt, dtype=np.uint8))
            if self._up_done[slot] is not None:
                self._up_done[slot].synchronize()
            pin = self._buf(self._pin_in, slot, a.shape, True)
            pin.copy_(a)
            if t is not None:
                pin_t = self._buf(self._pin_tgt, slot, t.shape, True)
                pin_t.copy_(t)
            with torch.cuda.stream(self.up):
                if self._consumed[slot] is not None:
                    self.up.wait_event(self._consumed[slot])
                old, old_t = self._dev_in[slot], self._dev_tgt[slot]
                if (old is None or tuple(old.shape) != tuple(a.shape)
                        or (t is not None and (old_t is None or tuple(old_t.shape) != tuple(t.shape)))):
                    self.up.wait_stream(main)
                dev = self._buf(self._dev_in, slot, a.shape, False)
                dev.copy_(pin, non_blocking=True)
                dev_t = None
                if t is not None:
                    dev_t = self._buf(self._dev_tgt, slot, t.shape, False)
                    dev_t.copy_(pin_t, non_blocking=True)
                ev = torch.cuda.Event(); ev.record(self.up)
            dev.record_stream(main)
            if dev_t is not None:
                dev_t.record_stream(main)
            self._up_done[slot] = ev
            return (dev, dev_t), ev

        nxt = next(it, None)
        slot = 0
        if nxt is not None:
            uploaded = upload(nxt, slot)
        while uploaded is not None:
            (dev, dev_t), ev = uploaded
            nxt = next(it, None)
            uploaded = upload(nxt, slot ^ 1) if nxt is not None else None     # overlaps with the forward below
            main.wait_event(ev)
            h, w = dev.shape[:2]
            x = self.ops.image_pre_u8(dev, self.window, self.swap_rb)
            if dev_t is None:
                c = torch.cuda.Event(); c.record(main)
                self._consumed[slot] = c               # dev_in[slot] may be overwritten by the upload stream after this
            y = self.net.restoration_network(x)
            res = self.ops.image_post_u8(y, h, w, self.swap_rb)
            met = None
            if dev_t is not None:
                met = self.ops.psnr_ssim_y(res, dev_t, crop_border, layout="HWC", bgr=self.swap_rb)
                c = torch.cuda.Event(); c.record(main)
                self._consumed[slot] = c               # dev_in[slot] and dev_tgt[slot] are free after the metric kernels
            done = torch.cuda.Event(); done.record(main)
            pin_out = self._buf(self._pin_out, slot, res.shape, True)
            pin_met = None if met is None else self._buf(self._pin_met, slot, (2,), True, torch.float64)
            with torch.cuda.stream(self.down):
                self.down.wait_event(done)
                pin_out.copy_(res, non_blocking=True)
                res.record_stream(self.down)
                if met is not None:
                    pin_met.copy_(met[0], non_blocking=True)
                    met.record_stream(self.down)
                dl = torch.cuda.Event(); dl.record(self.down)
            pending.append((pin_out, pin_met, dl))
            if len(pending) == 2:                      # the slot about to be reused must have been handed out
                yield self._hand_out(*pending.pop(0))
            slot ^= 1
        for p in pending:
            yield self._hand_out(*p)

    def _groups(self, items, scored):
        """Consecutive (image, target) items of equal shape, at most `batch` at a time, as lists of contiguous uint8 arrays."""
        import numpy as np
        group = []
        for item in items:
            img, tgt = item if scored else (item, None)
            a = np.ascontiguousarray(img)
            t = None if tgt is None else np.ascontiguousarray(tgt, dtype=np.uint8)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"UInt8Pipeline.run: expected (h, w, 3) uint8 images, got {a.shape} {a.dtype}")
            if t is not None and t.shape != a.shape:
                raise ValueError(f"UInt8Pipeline.run: target shape {t.shape} != image shape {a.shape}")
            if group and group[0][0].shape != a.shape:
                yield group
                group = []
            group.append((a, t))
            if len(group) == self.batch:
                yield group
                group = []
        if group:
            yield group

    def _plan(self, key):
        plan = self._plans.get(key)
        if plan is None:
            while len(self._plans) >= self.max_plans:
                torch.cuda.synchronize(self.device)    # nothing of a plan is freed under a copy or a replay that uses it
                self._plans.popitem(last=False)
            plan = self._plans[key] = _BatchPlan(self, *key[:3], *key[4:])
        else:
            self._plans.move_to_end(key)
        return plan

    def _run_batched(self, images, targets, crop_border):
        """run() with batch > 1, ensemble or graphed: the loop of run() over groups of images, a _BatchPlan per group."""
        main = torch.cuda.current_stream(self.device)
        scored = targets is not None
        groups = self._groups(iter(images) if not scored else zip(images, targets, strict=True), scored)
        pending = []                                   # (plan, images in it, download-done event)

        def upload(group, slot):
            """Stage a group into its plan: host -> pinned -> device on the upload stream, with run()'s orderings - the host refills
            the pinned buffers only after the previous copies out of them, the copies into the device buffers wait for main's last
            launch that read them (for main itself on the first use: the plan's memory is main's)."""
            h, w = group[0][0].shape[:2]
            with torch.cuda.device(self.device):
                plan = self._plan((h, w, len(group), slot, scored, crop_border))
            if plan.up_done is not None:
                plan.up_done.synchronize()
            for b, (a, t) in enumerate(group):
                plan.pin_in[b].copy_(torch.from_numpy(a))
                if t is not None:
                    plan.pin_tgt[b].copy_(torch.from_numpy(t))
            with torch.cuda.stream(self.up):
                if plan.consumed is not None:
                    self.up.wait_event(plan.consumed)
                else:
                    self.up.wait_stream(main)
                plan.dev_in.copy_(plan.pin_in, non_blocking=True)
                if scored:
                    plan.dev_tgt.copy_(plan.pin_tgt, non_blocking=True)
                ev = torch.cuda.Event(); ev.record(self.up)
            plan.up_done = ev
            return plan, len(group)

        slot = 0
        nxt = next(groups, None)
        staged = upload(nxt, slot) if nxt is not None else None
        while staged is not None:
            plan, count = staged
            nxt = next(groups, None)
            staged = upload(nxt, slot ^ 1) if nxt is not None else None       # overlaps with the forward below
            main.wait_event(plan.up_done)
            if plan.dl_done is not None:
                main.wait_event(plan.dl_done)          # the plan's previous results have left res (and the graph's metrics)
            met = plan.launch(self)
            c = torch.cuda.Event(); c.record(main)
            plan.consumed = c                          # dev_in and dev_tgt may be overwritten by the upload stream after this
            with torch.cuda.stream(self.down):
                self.down.wait_event(c)
                plan.pin_out.copy_(plan.res, non_blocking=True)
                if met is not None:
                    plan.pin_met.copy_(met, non_blocking=True)
                    if not self.graphed:
                        met.record_stream(self.down)
                dl = torch.cuda.Event(); dl.record(self.down)
            plan.dl_done = dl
            pending.append((plan, count, dl))
            if len(pending) == 2:                      # the slot about to be reused must have been handed out
                yield from self._hand_out_group(*pending.pop(0))
            slot ^= 1
        for p in pending:
            yield from self._hand_out_group(*p)

    @staticmethod
    def _hand_out_group(plan, count, done):
        done.synchronize()
        for b in range(count):
            img = plan.pin_out[b].numpy().copy()
            if plan.pin_met is None:
                yield img
            else:
                psnr, ssim = plan.pin_met[b].tolist()
                yield img, psnr, ssim

    @staticmethod
    def _hand_out(pin_out, pin_met, done):
        done.synchronize()
        img = pin_out.numpy().copy()
        if pin_met is None:
            return img
        psnr, ssim = pin_met.tolist()
        return img, psnr, ssim


def evaluate(net, device, images, targets, crop_border=1, swap_rb=True, batch=1, ensemble=False, graphed=False):
    """The reference's evaluation loop (inference_wavemamba.py:99-135) on host uint8 images (BGR, as cv2 reads them; RGB with
    swap_rb=False) and their ground truths: enhance every image on `device` (UInt8Pipeline) and score it on the device with
    the Y-channel PSNR / SSIM of comput_psnr_ssim.py (metrics.py).  LPIPS (:118-123) is not computed.
    batch, ensemble, graphed: UInt8Pipeline's switches (images per forward, geometric self-ensemble, graph replay).
    -> {"psnr": [...], "ssim": [...], "avg_psnr": mean, "avg_ssim": mean} (the averages :133-134 print)."""
    psnr, ssim = [], []
    pipe = UInt8Pipeline(net, device, swap_rb=swap_rb, batch=batch, ensemble=ensemble, graphed=graphed)
    for _, p, s in pipe.run(images, targets, crop_border):
        psnr.append(p)
        ssim.append(s)
    n = max(len(psnr), 1)
    return {"psnr": psnr, "ssim": ssim, "avg_psnr": sum(psnr) / n, "avg_ssim": sum(ssim) / n}


# ------------------------------------------------------------------------------------------------------------------
# bf16-storage mode (BASELINE config 2 as worded; ops.set_plane_dtype)
# ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def bench_bf16_storage(net, x, steps, warmup=2):
    """Time `steps` forwards with the LFSSBlock-internal planes stored as bfloat16 (fp32 arithmetic and state inside
    every kernel, fp32 tokens between blocks, fp32 HFE branch) and compare with the fp32 forward of the same input:
    PSNR on [0, 1]-clamped float outputs, PSNR after the reference's uint8 quantisation, relative l2."""
    import time
    from . import ops
    prev = ops.set_plane_dtype(torch.float32)
    try:
        ref = net.restoration_network(x)
        ops.set_plane_dtype(torch.bfloat16)
        for _ in range(max(warmup, 1)):
            out = net.restoration_network(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = net.restoration_network(x)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        ops.set_plane_dtype(prev)
    mse = float((out.clamp(0, 1) - ref.clamp(0, 1)).double().pow(2).mean())
    return {"images_per_s": steps / dt, "ms_per_step": 1e3 * dt / steps,
            "psnr_vs_fp32_db": float("inf") if mse == 0 else float(10 * torch.log10(torch.tensor(1.0 / mse))),
            "psnr_u8_vs_fp32_db": psnr_uint8(to_uint8(out), to_uint8(ref)),
            "rel_l2_vs_fp32": float((out - ref).norm() / ref.norm()),
            "note": "bf16 planes between the kernels of every LFSSBlock (x, z, conv outputs, the four scan outputs, f, fc); "
                    "fp32 tiles / projections / scan state / statistics inside the kernels, fp32 tokens, fp32 HFE branch"}
