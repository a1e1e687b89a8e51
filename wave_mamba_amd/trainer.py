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


def make_optimizer(net, lr=5e-4, weight_decay=1e-3, betas=(0.9, 0.99), capturable=False, backend="torch", ema_decay=None):
    """AdamW as the reference configures it (train_wavemamba_uhdll.yml:75-79).  On a GPU the 591 small tensors are
    updated by the fused multi-tensor implementation (one launch per ~hundred tensors instead of ~10 per tensor
    group); same arithmetic.  capturable: step counters AND the learning rate on the device, for GraphedTrainStep - a
    Python-float lr would be baked into the captured AdamW launch as a kernel scalar and a scheduler (the reference's recipe
    uses CosineAnnealingRestartCyclicLR, train_wavemamba_uhdll.yml:86-90: schedulers.py) would change nothing in the replays;
    schedulers.py and torch's own schedulers `fill_()` a tensor lr in place, which the replayed kernel reads (a warm-up or any
    other direct change goes through schedulers.set_lr, never `group["lr"] = value`).
    backend: "torch" (the default: everything above, and every call launches what it always launched) or "hip" - HipAdamW, this
    package's table-driven kernel, always capturable on a GPU.  ema_decay (backend "hip" only): keep an exponential moving average
    of the weights inside the optimizer's kernel (HipAdamW)."""
    if backend not in ("torch", "hip"):
        raise ValueError(f"make_optimizer: backend {backend!r} is not one of ('torch', 'hip')")
    params = [p for p in net.parameters() if p.requires_grad]
    if backend == "hip":
        return HipAdamW(params, lr=lr, weight_decay=weight_decay, betas=betas, ema_decay=ema_decay)
    if ema_decay is not None:
        raise ValueError("make_optimizer: ema_decay needs backend='hip' (the average is kept by HipAdamW's kernel)")
    fused = bool(params) and all(p.is_cuda for p in params)
    kw = {"capturable": True} if capturable else {}
    if capturable and fused:
        lr = torch.tensor(float(lr), dtype=torch.float32, device=params[0].device)
    return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, betas=betas, fused=fused, **kw)


class _AdamwGroup:
    """One param group's device state behind HipAdamW: three flat fp32 arenas (every tensor's slot starts on a 16-byte boundary),
    the per-parameter views of them, the step counter and the tables of addresses built so far."""

    def __init__(self, params, with_ema):
        self.params = params
        self.device = params[0].device
        sizes = [p.numel() for p in params]
        slots = [(n + 3) // 4 * 4 for n in sizes]
        self.sizes, self.slots = sizes, slots
        self.exp_avg, self.exp_avg_sq = self.arena(), self.arena()
        self.ema = self.arena() if with_ema else None
        self.m, self.v = self.views(self.exp_avg), self.views(self.exp_avg_sq)
        self.e = self.views(self.ema) if with_ema else None
        self.scratch = None                                        # swap_ema's, allocated at the first swap
        self.step = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.eager = (None, None)                                  # (gradient addresses, table): rebuilt when a gradient moved
        self.kept = {}                                             # gradient addresses -> table, for prepared and captured launches

    def arena(self):
        return torch.zeros(sum(self.slots), dtype=torch.float32, device=self.device)

    def views(self, flat):
        return [v[:n].view_as(p) for v, n, p in zip(flat.split(self.slots), self.sizes, self.params)]


class HipAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (amsgrad=False, maximize=False: both refused) whose step is this package's HIP kernel, with an optional
    exponential moving average of the weights computed in the same pass (the reference's model_ema, base_model.py:85-92;
    train.ema_decay of a BasicSR recipe).

        optimizer = HipAdamW(params, lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-3, ema_decay=0.999)      # or make_optimizer(backend="hip")
        ... optimizer.step() ...; optimizer.swap_ema(); validate(net); optimizer.swap_ema(); optimizer.ema_state_dict(net)

    On a GPU one step is ops.adamw_step per param group (the recipe has one): a launch over a device table of addresses
    {param, grad, exp_avg, exp_avg_sq, ema}, one workgroup per 4096 floats, plus one lane's counter increment.  The learning rate
    is a device tensor (schedulers.set_lr and the schedulers fill it in place) and the step counter is ONE float32 on the device, so
    the step is always capturable.  `found_inf` / `grad_scale` attributes (GradGuard.attach sets them) are read on the device: a step
    with found_inf set writes nothing, the counter included; with grad_scale the update uses grad / grad_scale, and - unlike
    torch's fused kernel - the divided gradients are NOT written back: p.grad keeps the unclipped values.
    exp_avg, exp_avg_sq and the average live in three flat fp32 arenas (every tensor's slot on a 16-byte boundary), all created
    here: moments and counter at 0, the average a copy of the weights.  The table is rebuilt when a gradient's address changed
    (eager steps); a captured step needs it before the capture: prepare(grads) with the tensors that will be p.grad (GraphedTrainStep
    and GraphedDDPTrainStep do that).  Parameters whose .grad is None are skipped.  CPU parameters (the gloo tests) run
    cpu_twin.adamw_step with a float lr: torch.optim.AdamW's single-tensor arithmetic, bit for bit.
    state_dict() has torch AdamW's keys - per parameter `step`, `exp_avg`, `exp_avg_sq`, and its group keys - so a training state
    written with either backend resumes with the other; load_state_dict copies INTO the arenas (the table holds their addresses) and
    refuses per-parameter `step` values that differ from each other.  The average is no part of that dict: ema_state_dict(net) /
    load_ema(state, net) / reset_ema() / swap_ema(), all in place."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, ema_decay=None):
        if amsgrad or maximize:
            raise ValueError("HipAdamW: amsgrad and maximize are not implemented")
        if isinstance(lr, torch.Tensor):
            lr = float(lr)
        if not (0.0 <= lr and 0.0 <= eps and 0.0 <= weight_decay and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"HipAdamW: lr {lr!r}, betas {betas!r}, eps {eps!r}, weight_decay {weight_decay!r}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"HipAdamW: ema_decay {ema_decay!r} does not lie in [0, 1)")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)         # torch AdamW's group keys, whatever the torch version
        defaults.update(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                        amsgrad=False, maximize=False, foreach=None, capturable=True, differentiable=False, fused=None)
        self._groups = None
        super().__init__(params, defaults)
        self._groups = []
        for group in self.param_groups:
            ps = group["params"]
            if not ps:
                raise ValueError("HipAdamW: a param group without parameters")
            if not all(p.dtype == torch.float32 and p.is_contiguous() and p.device == ps[0].device for p in ps):
                raise ValueError("HipAdamW: contiguous float32 parameters on one device per group")
            st = _AdamwGroup(ps, self.ema_decay is not None)
            self._groups.append(st)
            group["capturable"] = st.device.type == "cuda"       # (what a torch AdamW that loads this state will be told)
            if st.device.type == "cuda":
                group["lr"] = torch.tensor(float(group["lr"]), dtype=torch.float32, device=st.device)
            for p, m, v in zip(ps, st.m, st.v):
                self.state[p] = {"step": st.step.view(()), "exp_avg": m, "exp_avg_sq": v}
        self.reset_ema()

    def add_param_group(self, param_group):
        if self._groups is not None:
            raise RuntimeError("HipAdamW: param groups are fixed at construction (the arenas and tables are laid out there)")
        super().add_param_group(param_group)

    # -- the step ---------------------------------------------------------------------------------------------------------------
    def _build(self, st, grads):
        from . import ops
        rows = [(p, g, m, v, e) for p, g, m, v, e in zip(st.params, grads, st.m, st.v, st.e or [None] * len(st.params)) if g is not None]
        return ops.adamw_table(*[list(col) for col in zip(*rows)]) if rows else ops.adamw_table([], [], [], [])

    @staticmethod
    def _key(grads):
        return tuple(0 if g is None else g.data_ptr() for g in grads)

    def prepare(self, grads, group=0):
        """Build and keep the table for gradients at the addresses of `grads` (parallel to the group's parameters; None: no
        gradient) - outside a capture, for a step that will run inside one with exactly these tensors as p.grad."""
        st = self._groups[group]
        if st.device.type == "cuda":
            st.kept[self._key(grads)] = self._build(st, list(grads))

    def _table(self, st):
        grads = [p.grad for p in st.params]
        key = self._key(grads)
        capturing = torch.cuda.is_current_stream_capturing()
        table = st.kept.get(key)
        if table is None and st.eager[0] == key:
            table = st.eager[1]
            if capturing:
                st.kept[key] = table                               # a captured launch holds the table's address: never dropped
        if table is None:
            if capturing:
                raise RuntimeError("HipAdamW: no table for these gradient addresses - call prepare(grads) before the capture")
            table = self._build(st, grads)
            st.eager = (key, table)
        return table

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        found_inf, grad_scale = getattr(self, "found_inf", None), getattr(self, "grad_scale", None)
        for group, st in zip(self.param_groups, self._groups):
            if all(p.grad is None for p in st.params):
                continue
            if st.device.type == "cuda":
                from . import ops
                ops.adamw_step(self._table(st), group["lr"], st.step, group["betas"], group["eps"], group["weight_decay"],
                               self.ema_decay, found_inf, grad_scale)
                ops.conv2d_cache_clear()                           # the kernel writes through raw addresses: no `_version` moves
                continue
            if found_inf is not None and float(found_inf):
                continue
            from . import cpu_twin
            have = [i for i, p in enumerate(st.params) if p.grad is not None]
            cpu_twin.adamw_step([st.params[i] for i in have], [st.params[i].grad for i in have], [st.m[i] for i in have],
                                [st.v[i] for i in have], float(group["lr"]), int(st.step), group["betas"], group["eps"],
                                group["weight_decay"], None if st.e is None else [st.e[i] for i in have], self.ema_decay,
                                None if grad_scale is None else float(grad_scale))
            st.step += 1
        return loss

    # -- checkpoints ------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        state = super().state_dict()
        state["state"] = {k: {n: (t.detach().clone() if isinstance(t, torch.Tensor) else t) for n, t in s.items()}
                          for k, s in state["state"].items()}
        for g in state["param_groups"]:
            if isinstance(g["lr"], torch.Tensor):
                g["lr"] = g["lr"].detach().clone()
        return state

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups):
            raise ValueError("HipAdamW.load_state_dict: the number of param groups differs")
        for group, sg, st in zip(self.param_groups, saved, self._groups):
            if len(sg["params"]) != len(st.params):
                raise ValueError("HipAdamW.load_state_dict: a param group's size differs")
            if sg.get("amsgrad", False) or sg.get("maximize", False):
                raise ValueError("HipAdamW.load_state_dict: a state with amsgrad or maximize")
            states = [state_dict["state"].get(i) for i in sg["params"]]
            steps = sorted({float(s["step"]) for s in states if s is not None})
            if len(steps) > 1:
                raise ValueError(f"HipAdamW.load_state_dict: the parameters' step counts differ ({steps[0]:g} .. {steps[-1]:g}); "
                                 "this optimizer keeps one counter")
            for m, v, s in zip(st.m, st.v, states):
                if s is None:                                      # torch keeps no state for a parameter that never had a gradient
                    m.zero_()
                    v.zero_()
                else:
                    m.copy_(s["exp_avg"])
                    v.copy_(s["exp_avg_sq"])
            st.step.fill_(steps[0] if steps else 0.0)
            for k, value in sg.items():
                if k == "lr":
                    if isinstance(group["lr"], torch.Tensor):
                        group["lr"].fill_(float(value))
                    else:
                        group["lr"] = float(value)
                elif k == "betas":
                    group[k] = (float(value[0]), float(value[1]))
                elif k in ("eps", "weight_decay") or k not in self.defaults and k != "params":
                    group[k] = value                               # (initial_lr, lr_host: the schedulers' entries travel here)

    # -- the moving average -----------------------------------------------------------------------------------------------------
    def _need_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError(f"HipAdamW.{what}: no moving average is kept (ema_decay=None)")

    @torch.no_grad()
    def reset_ema(self):
        """The average becomes a copy of the current weights, in place (no-op without an ema_decay)."""
        for st in self._groups or []:
            if st.e is not None:
                torch._foreach_copy_(st.e, [p.detach() for p in st.params])

    def ema_arenas(self):
        """The flat tensors that hold the averages, one per param group (to snapshot and restore them in place)."""
        return [st.ema for st in self._groups if st.ema is not None]

    def ema_state_dict(self, net):
        """net.state_dict() with every parameter this optimizer updates taken from the average; buffers and frozen parameters come
        from the network.  Clones: the result does not follow later steps."""
        self._need_ema("ema_state_dict")
        net = _bare(net)
        state = {k: v.detach().clone() for k, v in net.state_dict().items()}
        by_param = {id(p): e for st in self._groups for p, e in zip(st.params, st.e)}
        for name, p in net.named_parameters():
            if id(p) in by_param and name in state:
                state[name] = by_param[id(p)].detach().clone()
        return state

    @torch.no_grad()
    def load_ema(self, state, net):
        """Fill the average from a state dict of the network (a file's `params_ema`), in place; a parameter the dict lacks keeps
        its average."""
        self._need_ema("load_ema")
        state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
        by_param = {id(p): e for st in self._groups for p, e in zip(st.params, st.e)}
        for name, p in _bare(net).named_parameters():
            if id(p) in by_param and name in state:
                by_param[id(p)].copy_(state[name])

    @torch.no_grad()
    def swap_ema(self):
        """Exchange weights and average in place, through a scratch arena: no address changes, so tables and captured graphs stay
        valid.  Call it twice around a validation."""
        self._need_ema("swap_ema")
        for st in self._groups:
            if st.scratch is None:
                st.scratch = st.arena()
            st.scratch.copy_(st.ema)
            torch._foreach_copy_(st.e, [p.detach() for p in st.params])
            torch._foreach_copy_([p.detach() for p in st.params], st.views(st.scratch))


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
            if not isinstance(optimizer, HipAdamW) and not all(g.get("fused", False) for g in optimizer.param_groups):
                raise RuntimeError("GradGuard.attach: on a GPU the optimizer must be the fused AdamW (make_optimizer) or a HipAdamW: "
                                   "only their kernels read found_inf / grad_scale from the device")
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
    (loss_values() to log them).  `fft_backend`: as in train_step; the captured graph keeps the backend it was captured with.
    With a HipAdamW (always capturable), as with a guard, the captured step copies its gradients into one flat buffer allocated
    before the capture and steps on views of it: the optimizer's table of addresses is built there, outside the capture."""

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
        hip_adamw = isinstance(optimizer, HipAdamW)
        flat_grads = guard is not None or hip_adamw                # a HipAdamW's table needs gradient addresses before the capture too
        if flat_grads:
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
        if guard is not None:
            guard.attach(optimizer)
            from . import ops
            self.guard_table = ops.grad_guard_table([self.flat])      # kept: the captured launch holds the table's address
        if hip_adamw:
            at = 0
            for gi, g in enumerate(optimizer.param_groups):           # (the optimizer keeps its tables: one per param group)
                optimizer.prepare(views[at:at + len(g["params"])], group=gi)
                at += len(g["params"])
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
            if flat_grads:
                torch._foreach_copy_(views, [p.grad if p.grad is not None else torch.zeros_like(p) for p in params])
                for p, v in zip(params, views):
                    p.grad = v
            if guard is not None:
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
        if isinstance(optimizer, HipAdamW):
            # its table over the packed views (most of them start off a 16-byte boundary: the kernel's element-wise rows), built
            # once, before any capture; the warm-up and the eager form find it under the same addresses
            at = 0
            for gi, g in enumerate(optimizer.param_groups):
                optimizer.prepare(self.views[at:at + len(g["params"])], group=gi)
                at += len(g["params"])
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


def save_network(net, path, current_iter=-1, epoch=0, param_key="params", ema=None):
    """`{param_key: state_dict on the CPU without 'module.' prefixes, 'iter': int | 'latest', 'epoch': int}` -
    the file layout `inference_wavemamba.py:74` / `load_network` read.  Rank 0 only (`@master_only`, :214).
    `ema`: a state dict of averaged weights (HipAdamW.ema_state_dict) - written beside `params` as `params_ema`, the key the
    reference's load_network looks for first (base_model.py:298-315) and load_network(param_key="params_ema") reads; None
    (the default): the file is what it always was."""
    if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
        return None
    plain = lambda sd: {(k[7:] if k.startswith("module.") else k): v.detach().cpu() for k, v in sd.items()}
    blob = {param_key: plain(_bare(net).state_dict())}
    if ema is not None:
        blob["params_ema"] = plain(ema)
    _atomic_save({**blob, "iter": "latest" if current_iter == -1 else current_iter, "epoch": epoch}, path)
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
