"""Training from the reference's recipe (options/train_wavemamba_uhdll.yml): options, sampler, the iteration loop of
basicsr/train.py:197-264 with its checkpoint cadence, validation with best-model bookkeeping (femasr_model.py:187-303,
base_model.py:50-83) and exact resume - around the pieces this package already has (data.PairedPatchBatcher, trainer.train_step /
GraphedTrainStep, schedulers, ops.psnr_ssim_y).

    opt, derived = load_options("train_wavemamba_uhdll.yml", num_train=len(store))
    Trainer(opt, train_store, val_store, graphed=True, out_dir="experiments/run").run()

    python -m wave_mamba_amd.recipe -opt FILE --train-pairs DIR [--val-pairs DIR] [--eager] [--out-dir DIR]

    torchrun --nproc_per_node N -m wave_mamba_amd.recipe -opt FILE --train-pairs DIR ... [--dist-backend nccl|gloo] [--collective split|captured]

Data-parallel training (the reference's `--launcher pytorch`).  Under an initialised torch.distributed group of more than one rank
(or with distributed=True, on a one-rank group too) the step is trainer.GraphedDDPTrainStep on the bare module - graph A, one flat
all-reduce, graph B; its eager form when the loop is not graphed - and the loop keeps its promises across ranks: the constructor's
warm-up is undone on every rank (rank 0's parameters are broadcast BEFORE the snapshot), rank 0 alone writes train.log, models/ and
training_states/, the logged losses are the mean over ranks, a state holds every rank's batcher random state (collected
collectively when it is saved) and resumes exactly at its own world size, and validation is sharded: rank r scores pairs r,
r + world, ... into its rows of an (n, borders, 2) float64 matrix, one all-reduce (sum) fills in the zero rows and every rank adds
the rows in store order - the single-process score bit for bit, the same best-model decision on every rank.  Every rank holds the
whole stores.  Without a group `rank` and `world` reach the sampler and the seeds only.
Out of scope: decoding image files (pairs are uint8 arrays), TensorBoard / wandb, LPIPS (skipped with a warning), saving
validation images.

Validation metrics.  The reference scores with `pyiqa` (femasr_model.py:39), a package that is not in its tree.  Here `psnr` and
`ssim` are this project's metrics.py - the reference's own comput_psnr_ssim.py, Y channel, on the uint8 image that tensor2img
produces - computed on the device by ops.psnr_ssim_y.

The guarded step.  An optional block switches trainer.GradGuard on for whichever step form the loop uses (absent: nothing changes,
the log line's keys included):
    train:
      grad_guard:
        max_norm: 1.0        # or ~ : no clipping
        skip_nonfinite: true
Every print_freq line then carries `grad_norm` (the last step's) and `skipped_steps`, read with the losses; a step whose gradients
are not finite leaves weights and optimizer state as they are while the iteration and the lr schedule advance (the batch was
consumed); the training state carries `skipped_steps` beside the batch position (a state without it resumes at 0).

The optimizer's backend and the weights' moving average.  Two optional keys (absent: nothing changes, the files included):
    train:
      ema_decay: 0.999       # standard BasicSR; 0 or absent: off; needs the backend below
      optim_g:
        backend: hip         # trainer.HipAdamW: the table-driven HIP step; torch (default): torch's fused AdamW
With an ema_decay the optimizer's kernel keeps the reference's model_ema (base_model.py:85-92) in its own pass.  The average starts
at the weights the run starts from (after pretrained weights are loaded and rank 0's broadcast), the graphed constructor's warm-up
is undone for it as for the moments, every net_g_*.pth carries `params_ema` beside `params`, validation scores the averaged
weights (swapped in and out in place, as BasicSR validates with net_g_ema) and a resumed run takes the average from the weights
file's `params_ema`, so it continues exactly.

Graphed mode and "one loop iteration = one recipe iteration".  GraphedTrainStep's constructor runs three warm-up steps on a side
stream before it captures; they are real optimizer steps.  The loop saves weights, moments and step counters before the
constructor and restores them IN PLACE after it (the graph reads those very tensors), so the warm-up leaves no trace and every
iteration - the first one and the first one after a resume included - is one replay.
"""
import json
import logging
import math
import os

import torch
import torch.distributed as dist

from . import schedulers, trainer
from .data import DeviceImageStore, PairedPatchBatcher
from .registry import build_network

LOG = logging.getLogger("wave_mamba_amd")
_OPTIM_KEYS = ("type", "lr", "weight_decay", "betas", "backend")
_GUARD_KEYS = ("max_norm", "skip_nonfinite")


# ---- options ---------------------------------------------------------------------------------------------------------------------
def _get(opt, dotted, default=None):
    for key in dotted.split("."):
        if not isinstance(opt, dict) or opt.get(key) is None:
            return default
        opt = opt[key]
    return opt


def usable_metrics(opt, warn=False):
    """{name: {"type", "crop_border", "better"}} of val.metrics that this package computes.  `lpips` is skipped (warn=True: with a
    warning - Trainer gives it once, when it sets up its validation); anything else but psnr / ssim on the Y channel is refused with a ValueError that names the key."""
    out = {}
    for name, m in (_get(opt, "val.metrics", {}) or {}).items():
        kind = m.get("type")
        if kind == "lpips":
            if warn:
                LOG.warning("val.metrics.%s: type lpips is not computed here; the metric is skipped", name)
            continue
        if kind not in ("psnr", "ssim"):
            raise ValueError(f"val.metrics.{name}.type: {kind!r} is not implemented (psnr, ssim; lpips is skipped)")
        if not m.get("test_y_channel", False):           # the reference's metric package defaults to false as well
            raise ValueError(f"val.metrics.{name}.test_y_channel: false is not implemented - only the Y-channel {kind} "
                             "(comput_psnr_ssim.py) runs on the device; the 3-channel SSIM does not exist here")
        out[name] = {"type": kind, "crop_border": int(m.get("crop_border", 0)), "better": m.get("better", "higher")}
    return out


def guard_options(opt):
    """train.grad_guard -> the arguments of trainer.GradGuard, or None without the block (the step is then exactly the unguarded
    one).  max_norm: a positive finite number, or ~ / absent for no clipping; skip_nonfinite: a bool (default true).  Anything else
    is refused with a ValueError that names the key."""
    block = _get(opt, "train.grad_guard")
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f"train.grad_guard: {block!r} is not a mapping ({', '.join(_GUARD_KEYS)})")
    for key in block:
        if key not in _GUARD_KEYS:
            raise ValueError(f"train.grad_guard.{key}: not an argument of trainer.GradGuard ({', '.join(_GUARD_KEYS)})")
    max_norm = block.get("max_norm")
    if max_norm is not None:
        if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or not 0.0 < float(max_norm) < float("inf"):
            raise ValueError(f"train.grad_guard.max_norm: {max_norm!r} is not a positive finite number (~ for no clipping)")
        max_norm = float(max_norm)
    skip = block.get("skip_nonfinite", True)
    if not isinstance(skip, bool):
        raise ValueError(f"train.grad_guard.skip_nonfinite: {skip!r} is not true or false")
    return {"max_norm": max_norm, "skip_nonfinite": skip}


def fft_backend_option(opt):
    """train.fft_opt.backend (this project's key, optional): `hip` - the fused FFT loss (ops.fft_l1_mean) - or `torch`.  Absent ->
    None: the process default (ops.set_fft_loss / WM_FFT_LOSS), so a recipe without the key trains as it always did."""
    backend = _get(opt, "train.fft_opt.backend")
    if backend is not None and backend not in ("hip", "torch"):
        raise ValueError(f"train.fft_opt.backend: {backend!r} is not one of hip, torch")
    return backend


def optimizer_backend_options(opt):
    """(train.optim_g.backend, train.ema_decay) -> (backend, ema_decay) for trainer.make_optimizer.  backend: `torch` (also when
    absent) or `hip` - trainer.HipAdamW.  train.ema_decay (standard BasicSR): 0 or absent for off -> None; otherwise a number in
    [0, 1), and it needs backend: hip - the average is kept by that optimizer's kernel.  A ValueError names the key."""
    backend = _get(opt, "train.optim_g.backend", "torch")
    if backend not in ("torch", "hip"):
        raise ValueError(f"train.optim_g.backend: {backend!r} is not one of torch, hip")
    decay = _get(opt, "train.ema_decay")
    if decay is None:
        return backend, None
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
        raise ValueError(f"train.ema_decay: {decay!r} is not a number in [0, 1) (0 or absent: no moving average)")
    if float(decay) == 0.0:
        return backend, None
    if backend != "hip":
        raise ValueError(f"train.ema_decay: {decay!r} needs train.optim_g.backend: hip (the moving average is kept by "
                         "trainer.HipAdamW's kernel)")
    return backend, float(decay)


def check_options(opt):
    """Refuse up front what the loop cannot do; every ValueError names the offending key."""
    if opt.get("scale", 1) != 1:
        raise ValueError(f"scale: {opt.get('scale')!r} is not implemented - the recipe trains at scale 1")
    optim = _get(opt, "train.optim_g")
    if optim is None:
        raise ValueError("train.optim_g: missing")
    if optim.get("type") != "AdamW":
        raise ValueError(f"train.optim_g.type: {optim.get('type')!r} is not implemented (AdamW)")
    for key in optim:
        if key not in _OPTIM_KEYS:
            raise ValueError(f"train.optim_g.{key}: not an argument of trainer.make_optimizer ({', '.join(_OPTIM_KEYS)})")
    for key in ("network_g", "train.scheduler", "train.total_iter", "datasets.train.gt_size", "datasets.train.batch_size_per_gpu",
                "logger.print_freq", "logger.save_checkpoint_freq"):
        if _get(opt, key) is None:
            raise ValueError(f"{key}: missing")
    guard_options(opt)
    fft_backend_option(opt)
    optimizer_backend_options(opt)
    metrics = usable_metrics(opt)
    key_metric = _get(opt, "val.key_metric")
    if opt.get("val") is not None and key_metric is not None and key_metric not in metrics:
        raise ValueError(f"val.key_metric: {key_metric!r} is not one of the metrics computed here ({', '.join(metrics) or 'none'})")


def derive_iters(opt, num_train, world_size=1):
    """train.py:66-71 -> {"num_iter_per_epoch", "total_iters", "total_epochs"}."""
    ds = opt["datasets"]["train"]
    ratio = ds.get("dataset_enlarge_ratio", 1)
    per_epoch = math.ceil(num_train * ratio / (ds["batch_size_per_gpu"] * world_size))
    total_iters = int(opt["train"]["total_iter"])
    return {"num_iter_per_epoch": per_epoch, "total_iters": total_iters, "total_epochs": math.ceil(total_iters / per_epoch)}


def load_options(path_or_text, num_train=None, world_size=1):
    """The recipe as a dict (yaml.safe_load: the `!!float` tags of the shipped file are standard YAML), checked by check_options.
    `path_or_text`: a file name, or the YAML text itself (anything with a line break).  -> (opt, derived): derived is
    derive_iters(opt, num_train, world_size), or None while the number of training pairs is not known."""
    import yaml
    text = path_or_text
    if "\n" not in path_or_text:
        with open(path_or_text, encoding="utf-8") as f:
            text = f.read()
    opt = yaml.safe_load(text)
    if not isinstance(opt, dict):
        raise ValueError("load_options: the YAML document is not a mapping")
    check_options(opt)
    return opt, (None if num_train is None else derive_iters(opt, num_train, world_size))


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
class EnlargedSampler:
    """basicsr/data/data_sampler.py: ceil(n * ratio / num_replicas) indices per replica and epoch - torch.randperm of the enlarged
    range from a generator seeded with the epoch, % n, then every num_replicas-th index starting at `rank`.  `n` is the number of
    pairs (the reference takes the dataset and reads its length)."""

    def __init__(self, n, num_replicas=1, rank=0, ratio=1):
        self.n, self.num_replicas, self.rank, self.epoch = int(n), int(num_replicas), int(rank), 0
        self.num_samples = math.ceil(self.n * ratio / self.num_replicas)
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        g = torch.Generator()
        g.manual_seed(self.epoch)
        indices = [v % self.n for v in torch.randperm(self.total_size, generator=g).tolist()]
        return iter(indices[self.rank:self.total_size:self.num_replicas])

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch

    def batches(self, batch_size):
        """The epoch's batches: `batch_size` consecutive indices each, the last short one dropped (data/__init__.py:91)."""
        idx = list(self)
        return [idx[i:i + batch_size] for i in range(0, len(idx) - batch_size + 1, batch_size)]


# ---- best-model bookkeeping --------------------------------------------------------------------------------------------------------
class BestMetrics:
    """base_model.py:50-83 for one validation set.  A metric is `higher` unless it carries `better: lower`; a tie is an update.
    update(results, current_iter, key_metric) -> True when the best model is to be saved: with a key metric, when THAT metric
    was updated (every metric's record then takes this validation's value, femasr_model.py:277-288); without one, when any was."""

    def __init__(self, metrics):
        self.records = {name: {"better": m.get("better", "higher"),
                               "val": float("-inf") if m.get("better", "higher") == "higher" else float("inf"), "iter": -1}
                        for name, m in metrics.items()}

    def _update_best(self, name, val, current_iter):
        rec = self.records[name]
        if (val >= rec["val"]) if rec["better"] == "higher" else (val <= rec["val"]):
            rec["val"], rec["iter"] = val, current_iter
            return True
        return False

    def update(self, results, current_iter, key_metric=None):
        if key_metric is not None:
            if not self._update_best(key_metric, results[key_metric], current_iter):
                return False
            for name, val in results.items():
                self.records[name]["val"], self.records[name]["iter"] = val, current_iter
            return True
        return any([self._update_best(name, val, current_iter) for name, val in results.items()])


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
def _freq(value):
    return None if value is None else int(float(value))


class Trainer:
    """The reference's train_pipeline, for one process or for one rank of a torch.distributed group.

    opt          the recipe: a dict, a file name or YAML text (load_options)
    train_store  data.DeviceImageStore of the training pairs, on the device to train on (a 'cpu' store trains on the CPU)
    val_store    a store of whole validation pairs (H, W multiples of 8 as the arch's test() needs them, or padded up by reflection)
    graphed      True on a GPU: GraphedTrainStep through graphed_step_with_batcher, optimizer from make_optimizer(capturable=True);
                 False (and always on the CPU): train_step(..., as_float=False)
    step_fn      step_fn(lq, gt) -> {name: 0-dim tensor} in place of the step (tests)
    net          a ready network in place of build_network(opt["network_g"])
    distributed  None: the data-parallel mode (module docstring) is on exactly when torch.distributed is initialised with more than
                 one rank; True forces it on a one-rank group (the RCCL self-test; ValueError without a group); False: off
    process_group, collective   GraphedDDPTrainStep's (files are written by the group's rank 0, which save_network expects to be
                 the global rank 0)
    rank, world  in the mode they come from the group (explicit values that contradict it: ValueError); otherwise None reads as
                 0 / 1 and explicit values reach the sampler and the seeds only

    run(max_iters=None, on_iter=None) trains to the recipe's end; `max_iters` pauses after that many iterations (no end-of-training
    save / validation then; run() again continues).  on_iter(current_iter, epoch, lrs, rows, losses) is called after every step:
    host values, and the step's 0-dim device losses (valid until the next step).  Files: out_dir/models/net_g_{iter}.pth,
    net_g_latest.pth, net_g_best_{iter}.pth (net_g_best_.pth without a key metric), out_dir/training_states/{iter}.state,
    out_dir/train.log (one JSON object per line; the same lines go to the `wave_mamba_amd` logger)."""

    def __init__(self, opt, train_store, val_store=None, device=None, graphed=True, out_dir=".", rank=None, world=None, step_fn=None,
                 net=None, distributed=None, process_group=None, collective="split"):
        if not isinstance(opt, dict):
            opt, _ = load_options(opt)
        else:
            check_options(opt)
        ready = dist.is_available() and dist.is_initialized()
        if distributed is None:
            distributed = ready and dist.get_world_size(process_group) > 1
        elif distributed and not ready:
            raise ValueError("distributed: True needs an initialised torch.distributed process group")
        self.distributed, self.group, self.collective = bool(distributed), process_group, collective
        if self.distributed:
            for name, given, have in (("rank", rank, dist.get_rank(process_group)), ("world", world, dist.get_world_size(process_group))):
                if given is not None and int(given) != have:
                    raise ValueError(f"{name}: {given!r} contradicts the process group, where it is {have}")
            rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
        self.opt, self.train_store, self.val_store = opt, train_store, val_store
        self.rank, self.world = int(rank or 0), int(1 if world is None else world)
        self.writer = not self.distributed or self.rank == 0          # the rank that owns train.log, models/ and training_states/
        self.device = torch.device(device) if device is not None else train_store.device
        if self.device != train_store.device or (val_store is not None and val_store.device != self.device):
            raise ValueError(f"Trainer: the stores must live on the training device {self.device}")
        self.graphed = bool(graphed) and self.device.type == "cuda" and step_fn is None
        self.step_fn = step_fn
        self.out_dir = str(out_dir)
        ds, tr = opt["datasets"]["train"], opt["train"]
        seed = opt.get("manual_seed")
        self.batch_size = int(ds["batch_size_per_gpu"])
        self.fft_weight = float(_get(opt, "train.fft_opt.loss_weight", 0.1))
        self.fft_backend = fft_backend_option(opt)
        ssim = _get(opt, "train.pixel_ssim_opt.loss_weight")
        self.ssim_weight = None if ssim is None else float(ssim)
        self.warmup_iter = int(tr.get("warmup_iter", -1))
        self.print_freq, self.save_freq = _freq(opt["logger"]["print_freq"]), _freq(opt["logger"]["save_checkpoint_freq"])
        self.latest_freq = _freq(opt["logger"].get("save_latest_freq"))
        self.val_freq = _freq(_get(opt, "val.val_freq")) if val_store is not None and len(val_store) else None
        self.metrics = usable_metrics(opt, warn=True) if self.val_freq else {}
        self.key_metric = _get(opt, "val.key_metric") if self.metrics else None
        self.best = BestMetrics(self.metrics)

        if seed is not None:
            torch.manual_seed(int(seed) + self.rank)               # set_random_seed(seed + rank): the weights' initialisation
        self.net = (net if net is not None else build_network(opt["network_g"])).train().to(self.device)
        pretrained = _get(opt, "path.pretrain_network_g")
        resume_state = _get(opt, "path.resume_state")
        optim = tr["optim_g"]
        backend, self.ema_decay = optimizer_backend_options(opt)
        self.optimizer = trainer.make_optimizer(self.net, lr=float(optim["lr"]), weight_decay=float(optim.get("weight_decay", 1e-2)),
                                                betas=tuple(optim.get("betas", (0.9, 0.999))), capturable=self.graphed,
                                                backend=backend, ema_decay=self.ema_decay)
        schedulers.set_lr(self.optimizer, [float(optim["lr"])] * len(self.optimizer.param_groups))   # the exact float64 base lr
        self.scheduler = schedulers.build_scheduler(self.optimizer, tr["scheduler"])
        guard = guard_options(opt)
        self.guard = None if guard is None else trainer.GradGuard(**guard).attach(self.optimizer)
        self.sampler = EnlargedSampler(len(train_store), self.world, self.rank, ds.get("dataset_enlarge_ratio", 1))
        if self.sampler.num_samples < self.batch_size:
            raise ValueError(f"datasets.train.batch_size_per_gpu: {self.batch_size} is more than the {self.sampler.num_samples} "
                             "samples of an epoch - every batch would be dropped")
        self.batcher = PairedPatchBatcher(train_store, gt_size=int(ds["gt_size"]), geometric_augs=bool(ds.get("geometric_augs", False)),
                                          seed=None if seed is None else int(seed) + self.rank)
        derived = derive_iters(opt, len(train_store), self.world)
        self.total_iters, self.total_epochs = derived["total_iters"], derived["total_epochs"]
        self.last_iter = self.total_iters
        end = self.scheduler.last_iter()
        if end is not None and end < self.total_iters:
            self.last_iter = end
            self._log({"warning": f"train.total_iter is {self.total_iters} but the schedule ends after sum(periods) = {end - 1}: "
                                  f"iteration {end} is the last one that can run; training ends there with its save and validation"},
                      logging.WARNING)
        self.current_iter, self.epoch, self._pos, self._finished = 0, 0, 0, False
        self._gstep = self._run_graphed = None
        self._ema_loaded = False

        if resume_state:                                           # before anything is captured
            self._resume(resume_state, pretrained)
        elif pretrained:
            trainer.load_network(self.net, pretrained, strict=bool(_get(opt, "path.strict_load", True)))
        if self.distributed:                                       # seeds differ by rank: rank 0's initialisation is the run's
            trainer.broadcast_parameters(self.net, self.group)
        if self.ema_decay is not None and not self._ema_loaded:    # the average starts at the weights the run starts from
            self.optimizer.reset_ema()

    # -- resume ---------------------------------------------------------------------------------------------------------------------
    def _resume(self, path, pretrained):
        """train.py:159-163 + base_model.py:359-373.  The weights come from path.pretrain_network_g or, without one, from
        models/net_g_{iter}.pth beside the state's folder (the layout this class writes).  With the state's "recipe" entry the
        run continues exactly: position inside the epoch and the batcher's random state; without one (a state the reference
        wrote) the epoch restarts at its first batch with a fresh random state, as in the reference.  A state written in the
        distributed mode also names its world size and holds one random state per rank: it continues exactly at that world size,
        every rank taking its own; at another one, or in a single process - and a single-process state in the mode - the epoch
        restarts like a reference state's (its batches are other ones)."""
        state = torch.load(path, map_location="cpu", weights_only=True)
        epoch, current_iter = trainer.resume_training(state, [self.optimizer], [self.scheduler])
        weights = pretrained or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(path))), "models", f"net_g_{current_iter}.pth")
        trainer.load_network(self.net, weights, strict=bool(_get(self.opt, "path.strict_load", True)) if pretrained else True)
        if self.ema_decay is not None:                             # the average continues from the file's params_ema where it has one
            blob = torch.load(weights, map_location="cpu", weights_only=True)
            if isinstance(blob, dict) and "params_ema" in blob:
                self.optimizer.load_ema(blob["params_ema"], self.net)
                self._ema_loaded = True
        self.epoch, self.current_iter = int(epoch), int(current_iter)
        extra = state.get("recipe")
        if self.guard is not None:                                 # (a state without the count, or one the reference wrote: 0)
            self.guard.set_skipped((extra or {}).get("skipped_steps", 0))
        exact = extra is not None and extra.get("world") == (self.world if self.distributed else None)
        if exact:
            self._pos = int(extra["batch"])
            rng = extra["rngs"][self.rank] if self.distributed else extra["rng"]
            self.batcher.rng.setstate((rng[0], tuple(rng[1]), rng[2]))
        self._log({"resumed": path, "epoch": self.epoch, "iter": self.current_iter, "exact": exact})

    # -- logging / files ------------------------------------------------------------------------------------------------------------
    def _log(self, record, level=logging.INFO):
        line = json.dumps(record)
        if self.writer:
            os.makedirs(self.out_dir, exist_ok=True)
            with open(os.path.join(self.out_dir, "train.log"), "a", encoding="utf-8") as f:
                f.write(line + "\n")
        LOG.log(level, line)

    def _model_path(self, label):
        return os.path.join(self.out_dir, "models", f"net_g_{label}.pth")

    def _save_network(self, label, current_iter, epoch):
        if self.writer:                                            # with train.ema_decay the file carries params and params_ema
            ema = None if self.ema_decay is None else self.optimizer.ema_state_dict(self.net)
            trainer.save_network(self.net, self._model_path(label), current_iter, epoch, ema=ema)

    def _all_rng_states(self):
        """Every rank's batcher random state, on every rank: each rank fills its row of a (world, 624 + 1) int64 matrix and one
        all-reduce (sum) fills in the others' (the collective both backends have for device and host tensors alike)."""
        version, words, gauss = self.batcher.rng.getstate()
        if gauss is not None:
            raise RuntimeError("Trainer: the batcher's random state holds a pending gauss() value; only randint() is drawn from it")
        mat = torch.zeros((self.world, len(words)), dtype=torch.int64, device=self.device)
        mat[self.rank] = torch.tensor(words, dtype=torch.int64)
        dist.all_reduce(mat, op=dist.ReduceOp.SUM, group=self.group)
        return [(version, tuple(row), None) for row in mat.tolist()]

    def save(self, epoch, current_iter):
        """model.save(): base_model.py:227-228 and :341-342 name the files.  In the distributed mode a collective: every rank
        calls it, rank 0 writes.  With train.grad_guard: a save that falls on a step whose found_inf was set is written like any
        other.  This is deliberate, and differs from the wording "a checkpoint is not written from a step whose found_inf is set":
        withholding the file would need a host read of found_inf at every save and would leave a hole in the save cadence that
        resume relies on (models/net_g_{iter}.pth beside training_states/{iter}.state), and it protects nothing - nothing of that
        step is in the file: the step was skipped, so the weights and the optimizer state are the previous
        step's, bit for bit - and the state carries the count of skipped steps ("skipped_steps", beside the batch position)."""
        extra = {"batch": self._pos, "rng": self.batcher.rng.getstate()}
        if self.distributed:
            extra = {"world": self.world, "batch": self._pos, "rngs": self._all_rng_states()}
        if self.guard is not None:
            extra["skipped_steps"] = int(self.guard.skipped)
        self._save_network("latest" if current_iter == -1 else current_iter, current_iter, epoch)
        if self.writer:
            trainer.save_training_state(os.path.join(self.out_dir, "training_states", f"{current_iter}.state"), epoch, current_iter,
                                        [self.optimizer], [self.scheduler], extra=extra)

    # -- the step ---------------------------------------------------------------------------------------------------------------------
    def _capture(self, lq, gt):
        """GraphedTrainStep on (lq, gt) whose three warm-up steps leave no trace (see the module docstring).  Distributed mode:
        GraphedDDPTrainStep, captured when the loop is graphed and in its eager form otherwise.  Its constructor broadcasts rank
        0's parameters before it warms up, so the broadcast comes first here: a snapshot taken before it would put a rank's own
        weights back."""
        if self.distributed:
            trainer.broadcast_parameters(self.net, self.group)
        params = [p for g in self.optimizer.param_groups for p in g["params"]]
        weights = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        moments = {p: {k: v.clone() for k, v in st.items() if isinstance(v, torch.Tensor)} for p, st in self.optimizer.state.items()}
        skipped = None if self.guard is None else int(self.guard.skipped)         # the warm-up steps are guarded steps too
        emas = [a.clone() for a in self.optimizer.ema_arenas()] if self.ema_decay is not None else []   # ... and averaged ones
        if self.distributed:
            step = trainer.GraphedDDPTrainStep(self.net, self.optimizer, lq, gt, process_group=self.group, capture=self.graphed,
                                               collective=self.collective, ssim_weight=self.ssim_weight, fft_weight=self.fft_weight,
                                               guard=self.guard, fft_backend=self.fft_backend)
        else:
            step = trainer.GraphedTrainStep(self.net, self.optimizer, lq, gt, ssim_weight=self.ssim_weight, fft_weight=self.fft_weight,
                                            guard=self.guard, fft_backend=self.fft_backend)
        if skipped is not None:
            self.guard.set_skipped(skipped)
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(weights[k])
            for p in params:
                saved = moments.get(p)
                for k, v in self.optimizer.state.get(p, {}).items():
                    if isinstance(v, torch.Tensor):
                        v.copy_(saved[k]) if saved is not None else v.zero_()    # no state before: exp_avg, exp_avg_sq, step = 0
            for a, saved in zip(self.optimizer.ema_arenas() if emas else [], emas):
                a.copy_(saved)                                     # the average is put back, never zeroed
        return step

    def _step(self, rows):
        if self.graphed or (self.distributed and self.step_fn is None):
            if self._gstep is None:
                self._gstep = self._capture(*self.batcher.form(rows=rows))
                self._run_graphed = trainer.graphed_step_with_batcher(self._gstep, self.batcher)
            return self._run_graphed(rows=rows)
        lq, gt = self.batcher.form(rows=rows)
        if self.step_fn is not None:
            return self.step_fn(lq, gt)
        return trainer.train_step(self.net, self.optimizer, lq, gt, as_float=False, ssim_weight=self.ssim_weight,
                                  fft_weight=self.fft_weight, guard=self.guard, fft_backend=self.fft_backend)

    # -- validation -------------------------------------------------------------------------------------------------------------------
    def _enhance_u8(self, lq):
        """(h, w, 3) uint8 BGR -> the network's output as tensor2img quantises it, (h, w, 3) uint8 BGR."""
        h, w = lq.shape[:2]
        if lq.is_cuda:
            from . import ops
            return ops.image_post_u8(self.net.test(ops.image_pre_u8(lq, 8, True)), h, w, True)
        from .inference import check_image_size, to_uint8
        x = lq.permute(2, 0, 1).flip(0)[None].float() / 255.0
        out = self.net.test(check_image_size(x, 8))[:, :, :h, :w]
        return to_uint8(out)[0].flip(0).permute(1, 2, 0).contiguous()

    @torch.no_grad()
    def score(self):
        """{metric: mean over val_store}: per pair net.eval(), the uint8 conversion, the arch's test() under no_grad, the
        tensor2img quantisation, the Y-channel PSNR / SSIM with the metric's crop_border, net.train() (femasr_model.py:187-199,
        :229-275).  On a GPU the per-image scores are summed on the device in float64, in store order, and read once."""
        borders = sorted({m["crop_border"] for m in self.metrics.values()})
        n = len(self.val_store)
        if not borders:
            return {}
        # (n, borders, 2): a pair's scores per border.  Distributed mode: rank r scores pairs r, r + world, ..., the other rows stay
        # zero and one all-reduce (sum) fills them in - adding zeros is exact, so every rank then holds the single-process rows
        rows = torch.zeros((n, len(borders), 2), dtype=torch.float64, device=self.device)
        for i in range(self.rank, n, self.world) if self.distributed else range(n):
            lq, gt = self.val_store.pair(i)
            self.net.eval()
            res = self._enhance_u8(lq)
            self.net.train()
            for j, c in enumerate(borders):
                if res.is_cuda:
                    from . import ops
                    rows[i, j] = ops.psnr_ssim_y(res, gt, c, layout="HWC", bgr=True)[0]
                else:
                    from .metrics import psnr_ssim_y_cpu
                    rows[i, j] = torch.tensor(psnr_ssim_y_cpu(res, gt, c, "HWC", True), dtype=torch.float64)
        if self.distributed:
            dist.all_reduce(rows, op=dist.ReduceOp.SUM, group=self.group)
        total = rows[0]
        for i in range(1, n):                                       # one row after the other, in store order: not a tree sum
            total = total + rows[i]
        host = dict(zip(borders, total.tolist()))
        return {name: host[m["crop_border"]][0 if m["type"] == "psnr" else 1] / n for name, m in self.metrics.items()}

    def validate(self, current_iter, epoch):
        """One validation: scores, best bookkeeping, the best checkpoint, one log line.  -> the result dict."""
        if self.ema_decay is not None:                             # the averaged weights are scored, as BasicSR does: swapped in
            self.optimizer.swap_ema()                              # and out again in place (addresses, tables and graphs stay)
        try:
            results = self.score()
        finally:
            if self.ema_decay is not None:
                self.optimizer.swap_ema()
        if self.best.update(results, current_iter, self.key_metric):
            self._save_network(f"best_{current_iter}" if self.key_metric is not None else "best_", current_iter, epoch)
        self._log({"iter": current_iter, "epoch": epoch, "validation": results,
                   "best": {k: {"val": r["val"], "iter": r["iter"]} for k, r in self.best.records.items()}})
        return results

    # -- train.py:197-264 ---------------------------------------------------------------------------------------------------------------
    def run(self, max_iters=None, on_iter=None):
        done = 0
        while not self._finished and self.epoch <= self.total_epochs:
            self.sampler.set_epoch(self.epoch)
            batches = self.sampler.batches(self.batch_size)
            while self._pos < len(batches):
                if max_iters is not None and done >= max_iters:
                    return {"iter": self.current_iter, "epoch": self.epoch, "finished": False}
                if self.current_iter + 1 > self.last_iter:
                    self._finished = True
                    break
                self.current_iter += 1
                it, epoch = self.current_iter, self.epoch
                schedulers.update_learning_rate([self.scheduler], [self.optimizer], it, self.warmup_iter)
                rows = self.batcher.draw(batches[self._pos])
                self._pos += 1
                losses = self._step(rows)
                done += 1
                if on_iter is not None:
                    on_iter(it, epoch, schedulers.current_lrs([self.optimizer]), rows, losses)
                if it % self.print_freq == 0:
                    guarded = {} if self.guard is None else {"grad_norm": float(self.guard.norm),
                                                             "skipped_steps": int(self.guard.skipped)}
                    self._log({"iter": it, "epoch": epoch, "lrs": schedulers.current_lrs([self.optimizer]),
                               **trainer.loss_values(losses), **guarded})
                if it % self.save_freq == 0 or (self.latest_freq and it % self.latest_freq == 0):
                    self.save(epoch, it)
                if self.val_freq and it % self.val_freq == 0:
                    self.validate(it, epoch)
            if self._finished:
                break
            self.epoch, self._pos = self.epoch + 1, 0
        self._finished = True
        self._save_network("latest", -1, -1)                                           # model.save(epoch=-1, current_iter=-1)
        last = self.validate(self.current_iter, self.epoch) if self.val_freq else None
        self._log({"end_of_training": True, "iter": self.current_iter})
        return {"iter": self.current_iter, "epoch": self.epoch, "finished": True, "validation": last}


# ---- command line ------------------------------------------------------------------------------------------------------------------
def load_pairs(folder, device):
    """DIR/lq/*.npy and DIR/gt/*.npy with equal names, each (h, w, 3) uint8 in BGR order -> DeviceImageStore on `device`."""
    import glob
    import numpy as np
    store = DeviceImageStore(device)
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(folder, "lq", "*.npy")))
    if not names:
        raise ValueError(f"{folder}: no lq/*.npy")
    for name in names:
        store.add(np.load(os.path.join(folder, "lq", name)), np.load(os.path.join(folder, "gt", name)))
    return store


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m wave_mamba_amd.recipe", description=__doc__.split("\n")[0])
    ap.add_argument("-opt", required=True, help="the recipe (YAML)")
    ap.add_argument("--train-pairs", required=True, help="folder with lq/*.npy and gt/*.npy (uint8, HWC, BGR)")
    ap.add_argument("--val-pairs", default=None)
    ap.add_argument("--eager", action="store_true", help="train_step per iteration instead of one graph replay")
    ap.add_argument("--out-dir", default="experiments")
    ap.add_argument("--device", default=None, help="default: cuda:0, under torchrun cuda:LOCAL_RANK")
    ap.add_argument("--max-iters", type=int, default=None, help="pause after this many iterations")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default=None, help="under torchrun; default: nccl on a GPU, gloo on the CPU")
    ap.add_argument("--collective", choices=("split", "captured"), default="split",
                    help="under torchrun, graphed: the all-reduce between two graph replays, or inside one graph (nccl only)")
    ap.add_argument("--dist-timeout", type=float, default=1800.0,
                    help="seconds after which a collective whose peer is gone ends with an error instead of waiting on")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    env = os.environ
    launched = all(k in env for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK")) and int(env["WORLD_SIZE"]) > 1
    device = torch.device(args.device or (f"cuda:{env['LOCAL_RANK']}" if launched else "cuda:0"))
    if launched:
        import datetime
        backend = args.dist_backend or ("nccl" if device.type == "cuda" else "gloo")
        if device.type == "cuda":
            torch.cuda.set_device(device)
        dist.init_process_group(backend, timeout=datetime.timedelta(seconds=args.dist_timeout),
                                **({"device_id": device} if backend == "nccl" else {}))
    try:
        train = load_pairs(args.train_pairs, device)
        val = load_pairs(args.val_pairs, device) if args.val_pairs else None
        opt, _ = load_options(args.opt, num_train=len(train))
        t = Trainer(opt, train, val, graphed=not args.eager, out_dir=args.out_dir, collective=args.collective)
        result = t.run(max_iters=args.max_iters)
        if t.writer:
            print(json.dumps(result))
    finally:
        if launched:
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
