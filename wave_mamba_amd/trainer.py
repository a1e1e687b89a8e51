"""Minimal trainer counterpart for the hot path's caller (reference basicsr/models/femasr_model.py).

Reproduces exactly what `FeMaSRModel.optimize_parameters` (:157-185) does to the network:
    loss = L1(output, gt) + 0.1 * L1(stack(rfft2(output).real/imag), stack(rfft2(gt).real/imag))
(`self.l1` is a bare nn.L1Loss :30,:171; FFTLoss losses.py:306-313 with fft_opt.loss_weight 0.1,
train_wavemamba_uhdll.yml:102-104; with `ssim_weight` the recipe's third term, ssim_weight * (1 - SSIM()(output, gt)),
cal_ssim.py / femasr_model.py:29, :172 / yml:99-100, joins the sum), AdamW(lr 5e-4, weight_decay 1e-3, betas (0.9, 0.99)) (yml:75-79),
DistributedDataParallel wrap with one gradient all-reduce per step (base_model.py:111-114; backend
'nccl' == RCCL on ROCm), and the per-iteration loss reduce to rank 0 (base_model.py:376-401).

Batches from images (data.py): the steps below take ready (B, 3, P, P) float32 `lq` / `gt`.  data.PairedPatchBatcher forms them on
the device from resident uint8 images, as the reference's PairedImageDataset train phase and collate would (crop, one of eight
flips / rotations, BGR -> RGB, CHW, / 255 - bit for bit), in one launch.  With a graphed step it writes straight into the graph's
input buffers, so no copy_ sits between the batch and the replay:

    step = GraphedTrainStep(net, optimizer, *batcher.form(first_indices))
    run = graphed_step_with_batcher(step, batcher)
    for indices in sampler:                            # B indices into the store per step
        losses = run(indices)                          # batcher.form(indices, out=(step.lq, step.gt)); step()
"""
import torch
import torch.distributed as dist
import torch.nn.functional as F


def _on_hip(a, b):
    return a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape


def l1(pred, target):
    """nn.L1Loss() (femasr_model.py:30, :171).  GPU fp32 tensors: the HIP reduction (ops.l1_mean) - no ATen semaphore memset in the
    step, so the step can be captured into a HIP graph and the REPORTED loss of a replay stays right."""
    if _on_hip(pred, target):
        from . import ops
        return ops.l1_mean(pred, target)
    return F.l1_loss(pred, target)


def fft_l1(pred, target, backend=None):
    """FFTLoss (losses.py:306-313): L1 between the stacked real/imag parts of rfft2.  On the GPU the same mean is taken over the
    interleaved (re, im) floats of the complex tensors (`view_as_real`: the stacked copies are never made).
    `backend`: None - the process default (ops.set_fft_loss / WM_FFT_LOSS; "torch" unless chosen otherwise) - "torch" or "hip".
    "hip" takes the fused kernels (ops.fft_l1_mean: one transform of pred - target, a fixed-order sum, no rocFFT plan and no
    spectrum tensor) for fp32 device tensors (B, C, H, W) whose H and W it has kernels for (ops.fft_l1_supported), and the path
    above for everything else, so a step never dies on a crop size."""
    from . import ops
    if backend is None:
        backend = ops.fft_loss_backend()
    elif backend not in ("torch", "hip"):
        raise ValueError(f"fft_l1: backend {backend!r} is not one of ('torch', 'hip')")
    if backend == "hip" and _on_hip(pred, target) and pred.dim() == 4 and ops.fft_l1_supported(pred.shape[2], pred.shape[3]):
        return ops.fft_l1_mean(pred, target)
    pf, tf = torch.fft.rfft2(pred), torch.fft.rfft2(target)
    if pf.is_cuda and pf.dtype == torch.complex64 and tf.dtype == torch.complex64:
        return l1(torch.view_as_real(pf), torch.view_as_real(tf))
    return F.l1_loss(torch.stack([pf.real, pf.imag], dim=-1), torch.stack([tf.real, tf.imag], dim=-1))


def ssim_loss(pred, target):
    """1 - SSIM()(pred, target): the recipe's SSIM term (self.ssim = SSIM().cuda(), femasr_model.py:29, its use at :172;
    cal_ssim.py:39-64; pixel_ssim_opt, train_wavemamba_uhdll.yml:99-100).  GPU fp32 tensors: the fused HIP forward / backward
    (ops.ssim_mean) - two launches and one per gradient, no ATen reduction, capturable like l1.  Anything else (CPU tensors, other
    dtypes): the plain-PyTorch statement of the same definition (cpu_twin.ssim_mean)."""
    if _on_hip(pred, target):
        from . import ops
        return 1 - ops.ssim_mean(pred, target)
    from . import cpu_twin
    return 1 - cpu_twin.ssim_mean(pred, target)


def losses(output, gt, fft_weight=0.1, ssim_weight=None, fft_backend=None):
    """(l_pix, l_freq), and with an `ssim_weight` (the recipe's is 0.25) a third term ssim_weight * ssim_loss.  `fft_backend`:
    fft_l1's `backend`."""
    if ssim_weight is None:
        return l1(output, gt), fft_weight * fft_l1(output, gt, fft_backend)
    return l1(output, gt), fft_weight * fft_l1(output, gt, fft_backend), ssim_weight * ssim_loss(output, gt)


_LOSS_NAMES = ("l_pix", "l_freq", "l_ssim")


def _total(terms):
    """The scalar that is differentiated: l_pix + l_freq, plus the weighted SSIM term where there is one."""
    total = terms[0] + terms[1]
    for t in terms[2:]:
        total = total + t
    return total.mean()


def make_optimizer(net, lr=5e-4, weight_decay=1e-3, betas=(0.9, 0.99), capturable=False):
    """AdamW as the reference configures it (train_wavemamba_uhdll.yml:75-79).  On a GPU the 591 small tensors are
    updated by the fused multi-tensor implementation (one launch per ~hundred tensors instead of ~10 per tensor
    group); same arithmetic.  capturable: step counters AND the learning rate on the device, for GraphedTrainStep - a
    Python-float lr would be baked into the captured AdamW launch as a kernel scalar and a scheduler (the reference's recipe
    uses CosineAnnealingRestartCyclicLR, train_wavemamba_uhdll.yml:86-90: schedulers.py) would change nothing in the replays;
    schedulers.py and torch's own schedulers `fill_()` a tensor lr in place, which the replayed kernel reads (a warm-up or any
    other direct change goes through schedulers.set_lr, never `group["lr"] = value`)."""
    params = [p for p in net.parameters() if p.requires_grad]
    fused = bool(params) and all(p.is_cuda for p in params)
    kw = {"capturable": True} if capturable else {}
    if capturable and fused:
        lr = torch.tensor(float(lr), dtype=torch.float32, device=params[0].device)
    return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, betas=betas, fused=fused, **kw)


def wrap_ddp(net, device=None, find_unused_parameters=False, force=False):
    """DDP wrap like base_model.py:111-114.  find_unused_parameters defaults to False: every one of
    the 591 parameter tensors receives a gradient, so the graph walk is wasted work.
    `force`: wrap at world size 1 as well (one-GPU self-tests of the RCCL path: the reducer then runs its bucketed
    all-reduce over a one-rank communicator)."""
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not force):
        return net
    ids = [device.index] if device is not None and device.type == "cuda" else None
    # gradient_as_bucket_view: the 591 gradients are views of the reducer's flat bucket instead of being copied into it
    # one small kernel at a time (measured over a one-rank RCCL communicator, config 3: see DESIGN.md section 6)
    return torch.nn.parallel.DistributedDataParallel(net, device_ids=ids, gradient_as_bucket_view=True,
                                                     find_unused_parameters=find_unused_parameters)


class GradGuard:
    """The guarded optimizer step: the global gradient norm, gradient clipping and the skip of a step whose gradients are not
    finite, decided ON THE DEVICE - so a captured step (GraphedTrainStep, GraphedDDPTrainStep) protects itself with the host out of
    the step.  One overflowing batch would otherwise write NaN into every weight and both Adam moments, and the replays would go on
    until somebody reads a loss.

        guard = GradGuard(max_norm=1.0)                      # max_norm=None: no clipping; skip_nonfinite=False: no skip
        step = GraphedTrainStep(net, optimizer, lq0, gt0, guard=guard)      # or train_step(..., guard=guard), GraphedDDPTrainStep
        ... float(guard.norm), int(guard.skipped)            # host reads: when logging, not every step

    On a GPU ops.grad_guard (two HIP launches: no atomics, no memset, bit-identical run to run) leaves {norm, found_inf, grad_scale}
    in `record`, and torch's fused AdamW reads two of them as `optimizer.found_inf` / `optimizer.grad_scale` (attach()): with
    found_inf == 1 its kernel leaves weights, both moments and the step counters as they are; with grad_scale = s it divides the
    gradients by s (in place) first, s = max(1, (norm + 1e-6) / max_norm) - torch.nn.utils.clip_grad_norm_, inverted.  `max_norm` is
    a launch scalar: a captured step keeps the value it was captured with.  CPU tensors (the gloo tests): cpu_twin.grad_guard
    decides on the host - the non-fused AdamW takes neither tensor.
    A skipped step leaves weights and optimizer state bit-equal and `skipped` one higher (counted only with skip_nonfinite); the
    batch is consumed, so the caller's iteration count and lr schedule advance.
    norm / found_inf / grad_scale: 0-dim views of `record`; skipped: 0-dim int64 - all of the last guarded step."""

    def __init__(self, max_norm=None, skip_nonfinite=True):
        if max_norm is not None and not (isinstance(max_norm, (int, float)) and not isinstance(max_norm, bool)
                                         and 0.0 < float(max_norm) < float("inf")):
            raise ValueError(f"GradGuard: max_norm {max_norm!r} (a positive finite number, or None for no clipping)")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.record = self._skipped = None
        self._captured_tables = []

    def to(self, device):
        """Allocate record and counter on `device` (kept, with their contents, when they live there already)."""
        device = torch.device(device)
        if self.record is None or self.record.device != device:
            count = 0 if self._skipped is None else int(self._skipped)
            self.record = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=device)
            self._skipped = torch.full((1,), count, dtype=torch.int64, device=device)
        return self

    norm = property(lambda self: self.record[0])
    found_inf = property(lambda self: self.record[1])
    grad_scale = property(lambda self: self.record[2])
    skipped = property(lambda self: self._skipped[0])

    def set_skipped(self, count):
        """Put the counter at `count`, in place (a resumed run)."""
        self._skipped.fill_(int(count))

    def attach(self, optimizer):
        """Allocate on the optimizer's device; on a GPU hand the fused AdamW its two device scalars (found_inf with
        skip_nonfinite, grad_scale with a max_norm).  Idempotent.  A CPU optimizer is left alone (the host decides: run())."""
        params = [p for g in optimizer.param_groups for p in g["params"]]
        if not params:
            raise ValueError("GradGuard.attach: the optimizer has no parameters")
        self.to(params[0].device)
        if self.record.is_cuda:
            if not all(g.get("fused", False) for g in optimizer.param_groups):
                raise RuntimeError("GradGuard.attach: on a GPU the optimizer must be the fused AdamW (make_optimizer): only its kernel "
                                   "reads found_inf / grad_scale from the device")
            if self.skip_nonfinite:
                optimizer.found_inf = self.found_inf
            if self.max_norm is not None:
                optimizer.grad_scale = self.grad_scale
        return self

    def run(self, grads, table=None):
        """Judge the gradients `grads` of one step; call between backward() and optimizer.step().  -> whether the caller calls
        optimizer.step(): always True on a GPU (the optimizer's kernel decides, from the record this launch leaves); for CPU
        tensors False for a step to skip, and the gradients are divided by grad_scale in place here.  `table`: the
        (table, n_rows) of ops.grad_guard_table over `grads`, built before a capture (this object then keeps it alive: the graph
        replays a launch on its address); None builds it now (not inside a capture)."""
        if self.record.is_cuda:
            from . import ops
            if table is not None and torch.cuda.is_current_stream_capturing():
                # a captured launch holds the ADDRESS of the device table: the table must outlive the graph, whoever built it
                if not any(t is table for t in self._captured_tables):
                    self._captured_tables.append(table)
            ops.grad_guard(table if table is not None else grads, self.max_norm, self.record,
                           self._skipped if self.skip_nonfinite else False)
            return True
        from . import cpu_twin
        self.record.copy_(cpu_twin.grad_guard(grads, self.max_norm))
        if self.skip_nonfinite and float(self.found_inf):
            self._skipped += 1
            return False
        if float(self.grad_scale) != 1.0:
            torch._foreach_div_(list(grads), float(self.grad_scale))
        return True


def _guard_grads(params):
    return [p.grad for p in params if p.grad is not None]


def train_step(net, optimizer, lq, gt, as_float=True, ssim_weight=None, fft_weight=0.1, guard=None, fft_backend=None):
    """One optimize_parameters(): zero_grad, forward, L1 + 0.1*FFT (+ ssim_weight * (1 - SSIM) where a weight is given; the
    loss dict then has "l_ssim", weighted like l_freq), backward (DDP all-reduce), step.
    Returns the reduced losses {name: python float} like the reference's `reduce_loss_dict` (base_model.py:376-401: a log dict
    of floats - callers format / json-dump it).  as_float=False returns 0-dim DEVICE tensors instead: nothing in the step then
    waits for the GPU (a `float()` is a host synchronisation per iteration, under DDP on every rank); `loss_values()` converts
    such a result when it is time to log (the reference logs every `print_freq` iterations).  bench.py and the tools time the
    step with as_float=False.  `fft_weight`: the recipe's fft_opt.loss_weight (train_wavemamba_uhdll.yml:102-104); `fft_backend`:
    which code computes that term (fft_l1's `backend`; None: the process default).
    `guard`: a GradGuard - after backward() it judges the parameters' gradients (the table of their addresses is rebuilt per
    call: eager gradients move), then the step is clipped or skipped as the guard says; the loss dict keeps its keys."""
    optimizer.zero_grad(set_to_none=True)
    out = net(lq)
    terms = losses(out, gt, fft_weight=fft_weight, ssim_weight=ssim_weight, fft_backend=fft_backend)
    _total(terms).backward()
    if guard is None or guard.attach(optimizer).run(_guard_grads([p for g in optimizer.param_groups for p in g["params"]])):
        optimizer.step()
    return reduce_loss_dict({k: t.detach() for k, t in zip(_LOSS_NAMES, terms)}, as_float=as_float)


class GraphedTrainStep:
    """train_step() captured ONCE into a HIP graph (forward, both losses, backward, AdamW) and replayed: a BASELINE config-3 step is
    ~2,500 kernel launches behind ~50 ms of Python and autograd bookkeeping - as much as the GPU needs for the kernels (54 ms), so on a
    host with slower cores the eager step waits for the host (60.6 against 54.8 ms of kernels on one box of the pool, round 5); a
    replay costs the host one call.  Single-process training only (GraphedDDPTrainStep is the data-parallel form: a
    DistributedDataParallel reducer cannot run inside a capture); fixed batch shape; `optimizer` must be make_optimizer(..., capturable=True): its learning rate is a device
    tensor, so a torch LR scheduler stepped between replays takes effect (it fills the tensor in place; a float lr is refused -
    it would be frozen into the graph).  The warm-up steps are real optimizer steps at the optimizer's current lr
    (recipe.Trainer undoes them in place, so that every iteration of its loop is one step of the recipe).

        step = GraphedTrainStep(net, optimizer, lq0, gt0)          # 3 eager warm-up steps on (lq0, gt0), then the capture
        losses = step(lq, gt)                                      # copies the batch into the graph's input buffers, replays
    Returns {"l_pix", "l_freq"} (and "l_ssim" with an `ssim_weight`) as 0-dim device tensors of the step just replayed
    (loss_values() to log them).  `fft_backend`: as in train_step; the captured graph keeps the backend it was captured with."""

    def __init__(self, net, optimizer, lq, gt, warmup=3, ssim_weight=None, fft_weight=0.1, guard=None, fft_backend=None):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("GraphedTrainStep: single-process training only (under torch.distributed: GraphedDDPTrainStep)")
        if not all(g.get("capturable", False) for g in optimizer.param_groups):
            raise RuntimeError("GraphedTrainStep: the optimizer must be capturable (make_optimizer(net, capturable=True))")
        if not all(isinstance(g["lr"], torch.Tensor) and g["lr"].is_cuda for g in optimizer.param_groups):
            raise RuntimeError("GraphedTrainStep: the optimizer's lr must be a device tensor (make_optimizer(net, capturable=True)): "
                               "a float lr is frozen into the captured graph and learning-rate schedules would be ignored")
        self.lq, self.gt = lq.clone(), gt.clone()
        self.lr_tensors = [g["lr"] for g in optimizer.param_groups]   # what the captured AdamW reads: fill_() them, never rebind g["lr"]
        side = torch.cuda.Stream(lq.device)
        side.wait_stream(torch.cuda.current_stream(lq.device))
        with torch.cuda.stream(side):                              # warm-up off the capture's stream (allocator pools, library set-up)
            for _ in range(warmup):
                train_step(net, optimizer, self.lq, self.gt, as_float=False, ssim_weight=ssim_weight, fft_weight=fft_weight, guard=guard,
                           fft_backend=fft_backend)
        torch.cuda.current_stream(lq.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        self.guard = guard
        if guard is not None:
            # the gradients of a capture live in the graph's pool; the guard's table holds addresses and its upload is a host-to-device
            # copy, so both are made HERE: one flat buffer the captured step copies its gradients into, per-parameter views of it as
            # the p.grad AdamW reads (GraphedDDPTrainStep's scheme), and one table over the whole buffer
            params = [p for g in optimizer.param_groups for p in g["params"]]
            # (every view starts on a 16-byte boundary, so the multi-tensor AdamW keeps its 16-byte accesses; the floats between
            # two views stay zero and add nothing to the norm, so one table over the whole buffer serves)
            sizes = [p.numel() for p in params]
            slots = [(n + 3) // 4 * 4 for n in sizes]
            self.flat = torch.zeros(sum(slots), dtype=torch.float32, device=lq.device)
            views = [v[:n].view_as(p) for v, n, p in zip(self.flat.split(slots), sizes, params)]
            guard.attach(optimizer)
            from . import ops
            self.guard_table = ops.grad_guard_table([self.flat])      # kept: the captured launch holds the table's address
        mode = {}
        if dist.is_available() and dist.is_initialized():
            # a (one-rank) process group exists: its watchdog thread polls events while this thread captures, which the default
            # global capture mode turns into a fatal error in the watchdog (see GraphedDDPTrainStep)
            torch.cuda.synchronize(lq.device)
            mode = {"capture_error_mode": "thread_local"}
        with torch.cuda.graph(self.graph, **mode):
            out = net(self.lq)
            terms = losses(out, self.gt, fft_weight=fft_weight, ssim_weight=ssim_weight, fft_backend=fft_backend)
            _total(terms).backward()
            if guard is not None:
                torch._foreach_copy_(views, [p.grad if p.grad is not None else torch.zeros_like(p) for p in params])
                for p, v in zip(params, views):
                    p.grad = v
                guard.run([self.flat], table=self.guard_table)
            optimizer.step()
        self.losses = {k: t.detach() for k, t in zip(_LOSS_NAMES, terms)}

    def __call__(self, lq=None, gt=None):
        if lq is not None:
            self.lq.copy_(lq)
        if gt is not None:
            self.gt.copy_(gt)
        self.graph.replay()
        return self.losses


def broadcast_parameters(net, process_group=None):
    """DDP's constructor: every rank of the group takes rank 0's parameters and buffers, in place."""
    src = dist.get_global_rank(process_group, 0) if process_group is not None else 0
    with torch.no_grad():
        for t in list(net.parameters()) + list(net.buffers()):
            dist.broadcast(t, src=src, group=process_group)


class GraphedDDPTrainStep:
    """The data-parallel optimize_parameters() (femasr_model.py:157-185 under the DistributedDataParallel wrap of
    base_model.py:111-114) with the host taken out of the step: every rank replays

        graph A   forward, both losses, backward, the 591 gradients (pre-divided by the world size, as DDP's reducer does)
                  and the two losses (three with an `ssim_weight`) copied into ONE flat fp32 buffer
        exchange  ONE all-reduce (sum) of that buffer - RCCL over xGMI: 6.05 MB per step for the shipped config
        graph B   AdamW on gradients that ARE views of the buffer

    instead of ~2,400 eager launches behind ~50 ms of Python, autograd and reducer bookkeeping per step and rank - with eight
    ranks on one host that work runs on whatever cores the host has left per rank (DESIGN.md section 6 has the measured host
    cost per step).  `net` is the BARE module (not the DDP wrap: the reducer's autograd hooks cannot run inside a capture); the
    constructor broadcasts rank 0's parameters and buffers like DDP's does.  `collective`:
        "split"     the all-reduce is an ordinary call between the two replays (any backend, gloo included)
        "captured"  one graph holds A, the all-reduce and B (backend nccl = RCCL only: its collectives are stream-ordered
                    kernels and capture like any other launch)
    `capture=False` runs the same three phases eagerly - what the CPU / gloo tests exercise, and the cross-check of the replays.
    Fixed batch shape; `optimizer` as for GraphedTrainStep on a GPU.  `ssim_weight`: the weighted SSIM term joins the sum and
    rides in the buffer as a third loss; `fft_weight`, `fft_backend`: the recipe's fft_opt.loss_weight and the code behind that term, as in GraphedTrainStep.  Returns {"l_pix", "l_freq"} (and "l_ssim" with an `ssim_weight`): 0-dim tensors holding the
    MEAN over ranks of the step just run (every rank has them - they ride in the gradient buffer; the reference's
    reduce_loss_dict, base_model.py:376-401, leaves them on rank 0 only)."""

    def __init__(self, net, optimizer, lq, gt, warmup=3, process_group=None, capture=True, collective="split", ssim_weight=None,
                 fft_weight=0.1, guard=None, fft_backend=None):
        if isinstance(net, (torch.nn.parallel.DistributedDataParallel, torch.nn.DataParallel)):
            raise RuntimeError("GraphedDDPTrainStep: pass the bare module, not its DistributedDataParallel wrap")
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("GraphedDDPTrainStep: torch.distributed is not initialised (single process: GraphedTrainStep)")
        if collective not in ("split", "captured"):
            raise ValueError("collective: 'split' or 'captured'")
        self.group = process_group
        self.world = dist.get_world_size(process_group)
        self.net, self.optimizer, self.capture, self.collective = net, optimizer, capture, collective
        self.ssim_weight, self.fft_weight, self.fft_backend = ssim_weight, fft_weight, fft_backend
        self.params = [p for g in optimizer.param_groups for p in g["params"]]
        if capture:
            if not all(p.is_cuda for p in self.params):
                raise RuntimeError("GraphedDDPTrainStep: capture needs the network on a GPU (capture=False runs eagerly)")
            if not all(g.get("capturable", False) and isinstance(g["lr"], torch.Tensor) and g["lr"].is_cuda
                       for g in optimizer.param_groups):
                raise RuntimeError("GraphedDDPTrainStep: the optimizer must be make_optimizer(net, capturable=True)")
            if collective == "captured" and dist.get_backend(process_group) != "nccl":
                raise RuntimeError("GraphedDDPTrainStep: collective='captured' needs the nccl (RCCL) backend")
        broadcast_parameters(net, process_group)
        dev = self.params[0].device
        self.sizes = [p.numel() for p in self.params]
        nl = 2 if ssim_weight is None else 3
        self.flat = torch.zeros(sum(self.sizes) + nl, dtype=torch.float32, device=dev)    # gradients | l_pix | l_freq (| l_ssim)
        self.views = [v.view_as(p) for v, p in zip(self.flat[:-nl].split(self.sizes), self.params)]
        self.losses = {k: self.flat[i - nl] for i, k in enumerate(_LOSS_NAMES[:nl])}
        self.lq, self.gt = lq.clone(), gt.clone()
        # the guard judges the REDUCED gradients (flat[:-nl]: the losses behind them are no part of the norm), so every rank takes
        # the same decision; the table over the buffer is built once, here, before any capture
        self.guard, self.guard_table = guard, None
        if guard is not None:
            guard.attach(optimizer)
            if dev.type == "cuda":
                from . import ops
                self.guard_table = ops.grad_guard_table([self.flat[:-nl]])
        self._grads = self.flat[:-nl]
        if not capture:
            return
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                              # warm-up off the capture's stream: real steps, all ranks alike
            for _ in range(warmup):
                self._produce()
                self._exchange()
                self._update()
        torch.cuda.current_stream(dev).wait_stream(side)
        # no collective of the warm-up may still be in flight, and the captures are THREAD-LOCAL: ProcessGroupNCCL's watchdog
        # thread polls its work events (hipEventQuery) while this thread captures; under the default global capture mode that
        # call is an error in the watchdog and ends the process
        torch.cuda.synchronize(dev)
        mode = {"capture_error_mode": "thread_local"}
        if collective == "captured":
            self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), None
            with torch.cuda.graph(self.graph_a, **mode):
                self._produce()
                self._exchange()
                self._update()
        else:
            self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_a, **mode):
                self._produce()
            with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool(), **mode):
                self._update()

    def _produce(self):
        for p in self.params:
            p.grad = None
        out = self.net(self.lq)
        terms = losses(out, self.gt, fft_weight=self.fft_weight, ssim_weight=self.ssim_weight, fft_backend=self.fft_backend)
        _total(terms).backward()
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in self.params]
        torch._foreach_copy_(self.views, grads)
        for k, t in zip(_LOSS_NAMES, terms):
            self.losses[k].copy_(t.detach())
        self.flat.mul_(1.0 / self.world)                           # DDP's reducer divides before it sums

    def _exchange(self):
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)

    def _update(self):
        for p, v in zip(self.params, self.views):
            p.grad = v
        if self.guard is None or self.guard.run([self._grads], table=self.guard_table):
            self.optimizer.step()

    def __call__(self, lq=None, gt=None):
        if lq is not None:
            self.lq.copy_(lq)
        if gt is not None:
            self.gt.copy_(gt)
        if not self.capture:
            self._produce()
            self._exchange()
            self._update()
        elif self.graph_b is None:
            self.graph_a.replay()
        else:
            self.graph_a.replay()
            self._exchange()
            self.graph_b.replay()
        return self.losses


def graphed_step_with_batcher(step, batcher):
    """The training loop's body for a GraphedTrainStep / GraphedDDPTrainStep fed by a data.PairedPatchBatcher: returns
    run(indices=None, rows=None), which forms the batch directly in the step's input buffers (one launch on the current stream,
    no copy_) and replays the step on them.  Returns the step's loss dict."""
    def run(indices=None, rows=None):
        batcher.form(indices, rows, out=(step.lq, step.gt))
        return step()
    return run


def loss_values(loss_dict):
    """{name: python float} of a train_step() result (synchronises: call it when logging, not every step)."""
    return {k: float(v) for k, v in loss_dict.items()}


def reduce_loss_dict(loss_dict, as_float=True):
    """base_model.py:376-401: sum-reduce to rank 0 then divide by world size (the values mean something on rank 0 only,
    as in the reference).  as_float=False keeps 0-dim tensors on their device (no host synchronisation)."""
    conv = (lambda v: float(v)) if as_float else (lambda v: v)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return {k: conv(v) for k, v in loss_dict.items()}
    keys = sorted(loss_dict)
    vec = torch.stack([loss_dict[k].float() for k in keys])
    dist.reduce(vec, dst=0)
    if dist.get_rank() == 0:
        vec /= dist.get_world_size()
    return {k: conv(v) for k, v in zip(keys, vec.unbind(0))}


# ---- reference-format checkpoints (basicsr/models/base_model.py:214-261, :299-326, :328-373) -----------------------
def _bare(net):
    return net.module if isinstance(net, (torch.nn.parallel.DistributedDataParallel, torch.nn.DataParallel)) else net


def _atomic_save(obj, path):
    """torch.save into a sibling temp file, then rename: a reader never sees a torn checkpoint (the reference retries
    the write three times instead, :247-260)."""
    import os
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def save_network(net, path, current_iter=-1, epoch=0, param_key="params"):
    """`{param_key: state_dict on the CPU without 'module.' prefixes, 'iter': int | 'latest', 'epoch': int}` -
    the file layout `inference_wavemamba.py:74` / `load_network` read.  Rank 0 only (`@master_only`, :214)."""
    if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
        return None
    state = {(k[7:] if k.startswith("module.") else k): v.detach().cpu() for k, v in _bare(net).state_dict().items()}
    _atomic_save({param_key: state, "iter": "latest" if current_iter == -1 else current_iter, "epoch": epoch}, path)
    return path


def load_network(net, path, strict=True, param_key="params", weights_only=True):
    """Counterpart of base_model.py:299-326: `param_key` falls back to 'params' when absent (None = the file is the
    bare state dict), 'module.' prefixes are dropped, and with strict=False tensors whose shape differs are skipped
    instead of raising.  Returns (missing_keys, unexpected_keys, skipped_for_shape).
    Reference-format files hold only tensors, ints, strs and (Ordered)dicts, so they load with `weights_only=True`
    (no arbitrary pickle code from a third-party checkpoint); pass weights_only=False for a trusted legacy file that
    pickles other objects."""
    blob = torch.load(path, map_location="cpu", weights_only=weights_only)
    if param_key is not None:
        if param_key not in blob and "params" in blob:
            param_key = "params"
        blob = blob[param_key]
    state = {(k[7:] if k.startswith("module.") else k): v for k, v in blob.items()}
    target = _bare(net)
    skipped = []
    if not strict:
        own = target.state_dict()
        skipped = sorted(k for k, v in state.items() if k in own and own[k].shape != v.shape)
        for k in skipped:
            del state[k]
    res = target.load_state_dict(state, strict=strict)
    from . import ops
    ops.conv2d_cache_clear()                 # prepared weight copies of the inference convolutions
    return list(res.missing_keys), list(res.unexpected_keys), skipped


def save_training_state(path, epoch, current_iter, optimizers, schedulers=(), extra=None):
    """`{'epoch', 'iter', 'optimizers': [...], 'schedulers': [...]}` (base_model.py:328-357); nothing is written for
    current_iter == -1, and only rank 0 writes.  `extra` (anything torch.load(weights_only=True) reads back) is stored under one
    more key, "recipe": recipe.Trainer keeps its position inside the epoch and the batcher's random state there; the reference's
    resume_training reads the four keys above and ignores the rest."""
    if current_iter == -1 or (dist.is_available() and dist.is_initialized() and dist.get_rank() != 0):
        return None
    state = {"epoch": epoch, "iter": current_iter, "optimizers": [o.state_dict() for o in optimizers],
             "schedulers": [s.state_dict() for s in schedulers]}
    if extra is not None:
        state["recipe"] = extra
    _atomic_save(state, path)
    return path


def resume_training(path_or_state, optimizers, schedulers=(), weights_only=True):
    """base_model.py:359-373.  Returns (epoch, iter).  `weights_only` as in load_network.
    A param group whose lr is a DEVICE tensor (make_optimizer(capturable=True)) keeps that tensor: optimizer.load_state_dict
    replaces the groups with the saved ones, whose lr is a CPU tensor (this package's files, loaded to the CPU) or a float (the
    reference's) - GraphedTrainStep refuses both, and a graph captured earlier would go on reading the old tensor.  The tensor is
    filled with the loaded value (its float64 mirror "lr_host" of schedulers.set_lr where the state has one) and put back."""
    st = path_or_state if isinstance(path_or_state, dict) else torch.load(path_or_state, map_location="cpu",
                                                                            weights_only=weights_only)
    if len(st["optimizers"]) != len(optimizers) or len(st["schedulers"]) != len(schedulers):
        raise ValueError("resume_training: optimizer / scheduler count differs from the saved state")
    for o, s in zip(optimizers, st["optimizers"]):
        kept = [g["lr"] if isinstance(g["lr"], torch.Tensor) and g["lr"].is_cuda else None for g in o.param_groups]
        o.load_state_dict(s)
        for g, lr in zip(o.param_groups, kept):
            if lr is not None:
                value = float(g["lr_host"]) if "lr_host" in g else float(g["lr"])
                lr.fill_(value)
                g["lr"], g["lr_host"] = lr, value
    for o, s in zip(schedulers, st["schedulers"]):
        o.load_state_dict(s)
    return st["epoch"], st["iter"]
