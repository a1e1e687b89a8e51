"""The reference's learning-rate schedules (basicsr/models/lr_scheduler.py) and its per-iteration update
(basicsr/models/base_model.py:126-140 setup_schedulers, :170-212 _set_lr / _get_init_lr / update_learning_rate /
get_current_learning_rate), for optimizers whose lr is a Python float OR a device tensor.

    MultiStepRestartLR(optimizer, milestones, gamma=0.1, restarts=(0,), restart_weights=(1,), last_epoch=-1)
    CosineAnnealingRestartLR(optimizer, periods, restart_weights=[1, 1], eta_min=0, last_epoch=-1)
    CosineAnnealingRestartCyclicLR(optimizer, periods, restart_weights, eta_mins=[0.0003, 0.000001], last_epoch=-1)
    build_scheduler(optimizer, opt)                    opt: the recipe's `train.scheduler` dict, 'type' included
    update_learning_rate(schedulers, optimizers, current_iter, warmup_iter=-1)
    set_lr(optimizer, values) / host_lr(group) / current_lrs(optimizers)

Why not the reference's classes as they are.  trainer.make_optimizer(capturable=True) keeps lr as a device tensor, because a
captured AdamW launch reads the tensor at every replay and would freeze a float.  Around such an optimizer torch's scheduler base
class clones the tensor into `base_lrs` and `_last_lr`, so the reference's formulas run in float32 on the device (a few ulp from
their float64 values), the state dict holds device tensors, and the reference's warm-up (`param_group['lr'] = value`) REBINDS the
entry: the replayed update goes on reading the old tensor and never sees the warm-up.  Here

  * every value is computed on the host in float64 from base learning rates captured as Python floats;
  * a float lr is assigned as the reference assigns it; a tensor lr is `fill_()`ed in place - one scalar fill, no
    synchronisation, never rebound - so it holds exactly the float32 rounding of the reference's float64 value;
  * the float64 value of a tensor lr is mirrored in its param group under "lr_host" (a float: it travels in the optimizer's
    state dict).  MultiStepRestartLR continues from the current lr and the log prints it; neither reads the device.  set_lr()
    on a fresh optimizer records the exact value (float(tensor) is only its float32 rounding);
  * state_dict() holds ints, floats, lists and dicts only (it loads under torch.load(weights_only=True)), under the reference's
    keys, and load_state_dict() takes a state the reference's class wrote (Counter milestones, tuples, tensor lrs);
  * past the last period the cosine schedules raise a ValueError that names the iteration and sum(periods) (the reference dies
    of a TypeError: get_position_from_periods returns None); last_iter() is the last iteration that can run.  The shipped recipe
    (total_iter 101000, periods [100, 100000]) reaches that point at iteration 100102.
"""
import math
from collections import Counter

import torch
from torch.optim.lr_scheduler import LRScheduler


def host_lr(group):
    """The float64 learning rate of a param group: the float itself, or the mirror set_lr() keeps beside a tensor lr.  A tensor
    without a mirror is read from the device (one synchronisation; its float32 value)."""
    lr = group["lr"]
    if not isinstance(lr, torch.Tensor):
        return float(lr)
    return float(group["lr_host"]) if "lr_host" in group else float(lr)


def set_lr(optimizer, values):
    """base_model.py:170-178 (_set_lr) for ONE optimizer: group i gets values[i].  A tensor lr is filled in place (and its float64
    value kept under "lr_host"), so a captured optimizer step reads the new value at its next replay; a float lr is rebound as
    in the reference."""
    groups = optimizer.param_groups
    if len(values) != len(groups):
        raise ValueError(f"set_lr: {len(values)} values for {len(groups)} param groups")
    for group, value in zip(groups, values):
        value = float(value)
        if isinstance(group["lr"], torch.Tensor):
            group["lr"].fill_(value)
            group["lr_host"] = value
        else:
            group["lr"] = value


def current_lrs(optimizers):
    """base_model.py:211-212 (get_current_learning_rate): the first group's lr of every optimizer, as host floats."""
    return [host_lr(o.param_groups[0]) for o in optimizers]


def _plain(v):
    """v as ints, floats, lists and dicts (tuples -> lists, Counter -> dict, 0-dim tensors -> floats)."""
    if isinstance(v, torch.Tensor):
        return float(v)
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


class _HostLRScheduler(LRScheduler):
    """Common part: float base lrs, host arithmetic, in-place update of tensor lrs, plain state."""

    def __init__(self, optimizer, last_epoch=-1):
        if last_epoch == -1:
            for group in optimizer.param_groups:
                group.setdefault("initial_lr", host_lr(group))     # a float: torch's base class would clone a tensor lr here
        super().__init__(optimizer, last_epoch)
        self.base_lrs = [float(v) for v in self.base_lrs]

    def step(self, epoch=None):
        self._step_count += 1
        self.last_epoch = self.last_epoch + 1 if epoch is None else int(epoch)
        values = [float(v) for v in self.get_lr()]
        set_lr(self.optimizer, values)
        self._last_lr = values

    def last_iter(self):
        """The last `current_iter` update_learning_rate() can be called with (None: no end)."""
        return None

    def state_dict(self):
        return {k: _plain(v) for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, state_dict):
        state = {k: _plain(v) for k, v in state_dict.items() if k != "optimizer"}
        self.__dict__.update(state)
        self._restore()

    def _restore(self):
        pass


class MultiStepRestartLR(_HostLRScheduler):
    """lr_scheduler.py:6-33.  At a restart the lr is initial_lr * its weight; at a milestone the CURRENT lr is multiplied by gamma
    (once per time the milestone is listed); otherwise it stays.  "Current" is what the group holds - after a warm-up that is
    the last warm-up value, as in the reference."""

    def __init__(self, optimizer, milestones, gamma=0.1, restarts=(0,), restart_weights=(1,), last_epoch=-1):
        self.milestones = Counter(milestones)
        self.gamma = gamma
        self.restarts = list(restarts)
        self.restart_weights = list(restart_weights)
        if len(self.restarts) != len(self.restart_weights):
            raise ValueError("MultiStepRestartLR: restarts and their weights do not match.")
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        groups = self.optimizer.param_groups
        if self.last_epoch in self.restarts:
            weight = self.restart_weights[self.restarts.index(self.last_epoch)]
            return [float(g["initial_lr"]) * weight for g in groups]
        if self.last_epoch not in self.milestones:
            return [host_lr(g) for g in groups]
        return [host_lr(g) * self.gamma ** self.milestones[self.last_epoch] for g in groups]

    def _restore(self):
        self.milestones = Counter({int(k): int(v) for k, v in self.milestones.items()})


def _position(last_epoch, cumulative_period, who):
    """lr_scheduler.py:36-54: the first period whose cumulative end is >= last_epoch."""
    for i, end in enumerate(cumulative_period):
        if last_epoch <= end:
            return i
    raise ValueError(f"{who}: last_epoch {last_epoch} (iteration {last_epoch + 1} of update_learning_rate) lies past the last "
                     f"period: sum(periods) = {cumulative_period[-1]}")


class _CosineRestart(_HostLRScheduler):
    def _cosine(self, eta_min_of):
        idx = _position(self.last_epoch, self.cumulative_period, type(self).__name__)
        weight = self.restart_weights[idx]
        nearest_restart = 0 if idx == 0 else self.cumulative_period[idx - 1]
        period = self.periods[idx]
        eta_min = eta_min_of(idx)
        return [eta_min + weight * 0.5 * (base_lr - eta_min) * (1 + math.cos(math.pi * ((self.last_epoch - nearest_restart) / period)))
                for base_lr in self.base_lrs]

    def last_iter(self):
        return self.cumulative_period[-1] + 1              # update_learning_rate(current_iter) evaluates last_epoch = current_iter - 1


class CosineAnnealingRestartCyclicLR(_CosineRestart):
    """lr_scheduler.py:57-106: cosine annealing with restarts and one eta_min per period (the recipe's schedule,
    train_wavemamba_uhdll.yml:86-90)."""

    def __init__(self, optimizer, periods, restart_weights, eta_mins=(0.0003, 0.000001), last_epoch=-1):
        self.periods = list(periods)
        self.restart_weights = list(restart_weights)
        self.eta_mins = list(eta_mins)
        if len(self.periods) != len(self.restart_weights):
            raise ValueError("CosineAnnealingRestartCyclicLR: periods and restart_weights should have the same length.")
        if len(self.eta_mins) < len(self.periods):
            raise ValueError("CosineAnnealingRestartCyclicLR: eta_mins needs one value per period.")
        self.cumulative_period = [sum(self.periods[0:i + 1]) for i in range(len(self.periods))]
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return self._cosine(lambda idx: self.eta_mins[idx])


class CosineAnnealingRestartLR(_CosineRestart):
    """lr_scheduler.py:108-147: cosine annealing with restarts and one eta_min.  As in the reference, the `restart_weights`
    argument is NOT used: the weights are [1, 1] (:130), so `periods` has two entries."""

    def __init__(self, optimizer, periods, restart_weights=(1, 1), eta_min=0, last_epoch=-1):
        self.periods = list(periods)
        self.restart_weights = [1, 1]
        self.eta_min = eta_min
        if len(self.periods) != len(self.restart_weights):
            raise ValueError("CosineAnnealingRestartLR: periods and restart_weights should have the same length.")
        self.cumulative_period = [sum(self.periods[0:i + 1]) for i in range(len(self.periods))]
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return self._cosine(lambda idx: self.eta_min)


_TYPES = {"MultiStepLR": MultiStepRestartLR, "MultiStepRestartLR": MultiStepRestartLR,
          "CosineAnnealingRestartLR": CosineAnnealingRestartLR, "CosineAnnealingRestartCyclicLR": CosineAnnealingRestartCyclicLR}


def build_scheduler(optimizer, opt):
    """base_model.py:126-140 for one optimizer: `opt` is the recipe's `train.scheduler` dict; its 'type' picks the class and the
    other entries are the constructor's keyword arguments.  (`opt` is not modified; the reference pops 'type'.)"""
    kwargs = dict(opt)
    name = kwargs.pop("type")
    if name not in _TYPES:
        raise NotImplementedError(f"Scheduler {name} is not implemented yet.")
    return _TYPES[name](optimizer, **kwargs)


def update_learning_rate(schedulers, optimizers, current_iter, warmup_iter=-1):
    """base_model.py:188-209.  Schedulers step only when current_iter > 1 (their constructor took the step of iteration 1); while
    current_iter < warmup_iter the lr is then overwritten with initial_lr / warmup_iter * current_iter, through set_lr()."""
    if current_iter > 1:
        for scheduler in schedulers:
            scheduler.step()
    if current_iter < warmup_iter:
        for optimizer in optimizers:
            set_lr(optimizer, [float(g["initial_lr"]) / warmup_iter * current_iter for g in optimizer.param_groups])
