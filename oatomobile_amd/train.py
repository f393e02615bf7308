"""DIM and CIL training steps on MI355X — `oatomobile/baselines/torch/dim/train.py:175-213` behind
the `rip_train_*` entry points of librip_hip.so (csrc/train.hip, csrc/flow.hip), and
`oatomobile/baselines/torch/cil/train.py:168-219` behind `rip_cil_train_*` (csrc/train.hip, csrc/cil.hip).

    trainer = DIMTrainer(model, lr=1e-3)                 # optim.Adam(model.parameters(), lr) (train.py:112-116)
    loss = trainer.train_step(batch)                     # train_step(model, optimizer, batch) (train.py:175-213)
    trainer.sync_to_model()                              # updated weights (and BN buffers) back into `model`
    loss = trainer.train_epoch(data, 512, generator=g)   # train_epoch (train.py:215-227) from a replay.DeviceCache

`batch` is what the reference's `transform` closure produces (train.py:122-134): `visual_features [B,C,100,100]`,
`velocity [B,3]`, `is_at_traffic_light [B,1]`, `traffic_light_state [B,1]`, `player_future [B,4,>=2]`, on the device.

Semantics are the reference's train mode: BatchNorm on batch statistics (running statistics updated with momentum
0.1), Dropout(0.2) in front of the MobileNetV2 classifier, the target perturbed with N(0, noise_level^2) noise
(train.py:184-189).  The two random draws come from torch's device generator; tests pass them in (`y=`,
`dropout_mask=`) to replay a step recorded from the reference.

Parameters, gradients and the Adam moments are single packed fp32 device tensors in the reference's state_dict order
(`arch.packed_spec`), so data-parallel training is one `all_reduce` of `trainer.grads` between `backward()` and
`apply()` (9.7 MB: the first bandwidth-relevant collective of this code base; only a trainer built with `group=`
reduces, and the averaged gradient — not the local one — is what `clip=True` clips).

`CILTrainer` is the same machinery for `BehaviouralModel` (cil/train.py): the same encoder and merger halves, the GRU
decoder's backward-through-time (`cil_train_kernel`) and the L1 loss in place of the flow; no target perturbation.

By default a step's sums over the batch are added with float atomics in three kernels, so two runs differ in the last
bits and drift apart over Adam steps.  `DIMTrainer(..., deterministic=True)` / `CILTrainer(..., deterministic=True)`
replace them with partial tables added in a fixed order: the same bits on every run (see the class docstrings for
what is and is not covered).
"""

import ctypes
from typing import Mapping, Optional

import numpy as np
import torch

from oatomobile_amd import _lib
from oatomobile_amd import arch
from oatomobile_amd.cil import BehaviouralModel
from oatomobile_amd.model import ImitativeModel

DROPOUT_P = 0.2  # torchvision MobileNetV2.classifier[0]


class _PackedTrainer:
  """What the DIM and CIL trainers share: one model, one device; the packed parameter / gradient / Adam-moment tensors
  in the model's state_dict order (`_state_dict_spec` minus the `num_batches_tracked` counters), the HIP workspace
  handle, and the step after `loss.backward()`: [all-reduce ->] [clip ->] Adam.  A subclass sets `_state_dict_spec`,
  creates the handle in `_create` and implements `backward`."""

  _state_dict_spec = None  # in_channels -> ordered [(key, shape)] of the model's state_dict

  def __init__(self, model, lr: float, weight_decay: float, max_batch: int, device: Optional[torch.device], betas,
               eps: float, group, deterministic: bool = False) -> None:
    name = type(self).__name__
    if not torch.cuda.is_available():
      raise RuntimeError("oatomobile_amd.%s needs a ROCm device; there is no CPU path." % name)
    self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if self._device.index is None:
      self._device = torch.device("cuda", torch.cuda.current_device())
    self._model = model
    self._C = model._in_channels
    self._lr, self._wd = float(lr), float(weight_decay)
    self._betas, self._eps = (float(betas[0]), float(betas[1])), float(eps)
    self._group = group
    if group is None and torch.distributed.is_available() and torch.distributed.is_initialized() \
        and torch.distributed.get_world_size() > 1:
      # torch's convention is group=None == the default WORLD group; here None means "do not reduce" (ranks that train
      # independent ensemble members).  Say so once instead of silently training unsynchronised replicas.
      import warnings
      warnings.warn("%s(group=None) in a %d-rank job: gradients are NOT all-reduced (independent replicas).  "
                    "Pass group=torch.distributed.group.WORLD for data-parallel training." %
                    (name, torch.distributed.get_world_size()), stacklevel=3)
    self._max_batch = int(max_batch)
    self._lib = _lib.load()
    self._h = ctypes.c_void_p(0)
    n = self._create()
    self._deterministic = False
    if deterministic:  # allocates the partial-sum workspace (about 25 MB)
      _lib.check(self._lib.rip_train_set_option(self._h, _lib.TRAIN_OPT_DETERMINISTIC, 1))
      self._deterministic = True
    spec_n = sum(int(np.prod(s)) if len(s) else 1 for _, s in self._packed_spec())
    if n != spec_n:
      raise RuntimeError("packed layout mismatch: library %d, state_dict spec %d" % (n, spec_n))
    mask = np.empty(n, np.uint8)
    _lib.check(self._lib.rip_train_trainable_mask(self._h, mask.ctypes.data_as(ctypes.c_void_p), n))
    self.params = torch.from_numpy(self._packed_weights(model)).to(self._device)
    self.grads = torch.zeros_like(self.params)
    self.exp_avg = torch.zeros_like(self.params)
    self.exp_avg_sq = torch.zeros_like(self.params)
    self._trainable = torch.from_numpy(mask).to(self._device)
    self._loss = torch.zeros((), device=self._device)
    self._last_batch = 0
    self.step_count = 0
    nbt = [v for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")]
    self.num_batches_tracked = int(nbt[0]) if nbt else 0  # nn.BatchNorm2d counts its train-mode forward passes

  def _create(self) -> int:
    """Creates `self._h`; returns the library's packed numel."""
    raise NotImplementedError

  @property
  def deterministic(self) -> bool:
    """Was this trainer built with `deterministic=True` (the same bits on every run; see the class docstring)."""
    return self._deterministic

  def _packed_spec(self):
    return [(k, s) for (k, s) in type(self)._state_dict_spec(self._C) if not k.endswith("num_batches_tracked")]

  def _packed_weights(self, model) -> np.ndarray:
    sd = model.state_dict()
    return np.concatenate([sd[k].detach().cpu().numpy().astype(np.float32).reshape(-1) for k, _ in self._packed_spec()])

  def _visual(self, batch: Mapping[str, torch.Tensor]) -> torch.Tensor:
    """`visual_features` as fp32 contiguous [B,C,100,100] on the device, B <= max_batch."""
    vis = batch["visual_features"]
    if not vis.is_cuda:
      raise RuntimeError("oatomobile_amd.%s: the batch is on %s — no CPU path" % (type(self).__name__, vis.device))
    vis = vis.detach().to(torch.float32).contiguous()
    _lib.expect_shape(vis, (None, self._C, arch.INPUT_HW, arch.INPUT_HW), "visual_features")
    if vis.shape[0] > self._max_batch:
      raise ValueError("batch of %d exceeds max_batch=%d" % (vis.shape[0], self._max_batch))
    return vis

  def _dropout_mask(self, B: int, train: bool, dropout_mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if train and dropout_mask is None:
      # keep with probability 1 - p, scaled by 1 / (1 - p) (nn.Dropout): two launches
      dropout_mask = torch.empty(B, arch.LAST_CHANNELS, device=self._device).bernoulli_(1.0 - DROPOUT_P).mul_(1.0 / (1.0 - DROPOUT_P))
    if dropout_mask is not None:
      dropout_mask = dropout_mask.to(self._device, torch.float32).contiguous()
      _lib.expect_shape(dropout_mask, (B, arch.LAST_CHANNELS), "dropout_mask")
    return dropout_mask

  # ---- after loss.backward(): the optimizer half of the reference's train_step ----
  def allreduce(self) -> None:
    """Data-parallel exchange: averages the packed gradient vector over the ranks of the `group` this trainer was
    built with (DistributedDataParallel semantics; BatchNorm running statistics stay per-rank buffers, there is no
    SyncBatchNorm).  Only a trainer that was GIVEN a group reduces: a job whose ranks train independent models
    (replay-sharded ensembles) keeps `group=None` and its gradients are never touched.  ONE all-reduce of 9.7 MB."""
    if self._group is None:
      return
    dist = torch.distributed
    with _lib.trace_range("rip all_reduce gradients (%d B)" % (self.grads.numel() * 4)):
      dist.all_reduce(self.grads, op=dist.ReduceOp.SUM, group=self._group)
    world = dist.get_world_size(self._group)
    if world > 1:
      self.grads /= world

  def clip_grad_norm(self, max_norm: float = 1.0) -> torch.Tensor:
    """train.py:207-208: `torch.nn.utils.clip_grad_norm(model.parameters(), 1.0)` on the packed gradient vector (the
    running-statistic slots hold zeros, so its 2-norm is the norm over the parameters).  Returns the norm."""
    norm = torch.linalg.vector_norm(self.grads)
    self.grads *= torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm

  def apply(self, clip: bool = False) -> None:
    """train.py:206-211: [all-reduce ->] [clip ->] `optimizer.step()` (torch.optim.Adam defaults).  The order is
    DistributedDataParallel's: the AVERAGED gradient is clipped, not each rank's local one."""
    self.allreduce()
    if clip:
      self.clip_grad_norm(1.0)
    self.step_count += 1
    _lib.check(self._lib.rip_train_adam(
        _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
        _lib.ptr(self._trainable, torch.uint8), self.params.numel(), self.step_count, self._lr, self._betas[0],
        self._betas[1], self._eps, self._wd, _lib.current_stream(self._device)))

  def peek(self, layer: int, what: str = "post") -> torch.Tensor:
    """What the last `backward` saved for conv layer `layer` (0 = features.0, ...), as NCHW: "pre" (conv output
    before BatchNorm), "post" (after BatchNorm / ReLU6 / residual) or "grad" (dLoss/dpost)."""
    spec = arch.conv_layers(self._C)[layer]
    B = self._last_batch
    buf = torch.empty(B, spec.h_out, spec.h_out, spec.cout, device=self._device)
    _lib.check(self._lib.rip_train_peek(self._h, layer, {"pre": 0, "post": 1, "grad": 2}[what], B, _lib.ptr(buf), buf.numel(),
                                        _lib.current_stream(self._device)))
    return buf.permute(0, 3, 1, 2)

  # ---- by the epoch, from a device-resident cache (replay.DeviceCache) ----
  _epoch_mode = False  # does the batch carry the CIL `mode`

  def _epoch_horizon(self) -> int:
    raise NotImplementedError

  def _target_noise(self, target: torch.Tensor, rows: int, a: int, b: int, generator) -> Optional[torch.Tensor]:
    """The perturbed target `y` of this rank's slice [a, b) of a global batch of `rows` rows, or None (no noise)."""
    return None

  def _rank_world(self):
    if self._group is None:
      return 0, 1
    return torch.distributed.get_rank(self._group), torch.distributed.get_world_size(self._group)

  def train_epoch(self, data, batch_size: int, *, generator: Optional[torch.Generator] = None, clip: bool = False) -> float:
    """One epoch of the reference's `train_epoch` (dim/train.py:215-228, cil/train.py:192-206) over `data`, a
    `replay.DeviceCache`: `DataLoader(shuffle=True, drop_last=False)` semantics, `train_step` per batch, and the
    mean of the per-batch losses (`loss / len(dataloader)`) as a float.

    The random draws come from `generator` (a generator on this trainer's device; None = torch's default one) in
    this order: `torch.randperm(len(data))` once (kept in `self.last_permutation`), then per batch the target noise
    N(0, noise_level^2) of shape [rows, T, 2] (DIM only) and the dropout keep mask (`bernoulli_(0.8)` of shape
    [rows, 1280], scaled by 1 / 0.8).  Per-batch losses stay on the device (`self.last_epoch_losses`); the epoch
    synchronises once, for its result.

    With `group=` (data parallel) every rank must pass an identically seeded generator: all ranks draw the same
    permutation, a global batch is `batch_size * world` rows and rank r trains on its `distributed.shard_range` slice
    of it.  The noise and the mask are drawn for the whole global batch and sliced, so the generators stay in step.
    The gradient is row-weighted: when the slices of a global batch are uneven (its last one), a rank scales its
    batch-mean gradient by `rows_r * world / rows` before the all-reduce averages it, so the reduced gradient is the
    mean over the global batch's rows, as one process would compute it (a rank with an empty slice contributes
    zero).  BatchNorm statistics are per rank, as under DistributedDataParallel without SyncBatchNorm.  The per-batch
    losses are row-weighted over the ranks too (one all-reduce at the end of the epoch), so every rank returns the
    same epoch loss."""
    from oatomobile_amd.distributed import shard_range
    if batch_size < 1 or batch_size > self._max_batch:
      raise ValueError("batch_size=%d outside [1, max_batch=%d]" % (batch_size, self._max_batch))
    if data.channels != self._C:
      raise ValueError("the cache has %d BEV channels, the model %d" % (data.channels, self._C))
    T = self._epoch_horizon()
    rank, world = self._rank_world()
    n = len(data)
    perm = torch.randperm(n, device=self._device, generator=generator)
    self.last_permutation = perm
    losses, global_rows = [], []
    gb = batch_size * world
    for g0 in range(0, n, gb):
      rows = min(gb, n - g0)
      a, b = shard_range(rows, rank, world)
      global_rows.append(rows)
      if b == a:
        self.grads.zero_()
        self.apply(clip=clip)
        losses.append(torch.zeros((), device=self._device))
        continue
      batch = data.batch(perm[g0 + a:g0 + b], T, mode=self._epoch_mode)
      y = self._target_noise(batch["player_future"], rows, a, b, generator)
      keep = torch.empty(rows, arch.LAST_CHANNELS, device=self._device).bernoulli_(1.0 - DROPOUT_P, generator=generator)
      keep = keep.mul_(1.0 / (1.0 - DROPOUT_P))[a:b]
      kw = {} if y is None else {"y": y}
      loss = self.backward(batch, dropout_mask=keep, **kw)
      if world > 1 and (b - a) * world != rows:  # uneven slices: row-weight this rank's share of the average
        self.grads.mul_((b - a) * world / rows)
      losses.append(loss * (b - a) if world > 1 else loss)
      self.apply(clip=clip)
    if not losses:
      self.last_epoch_losses = torch.zeros(0, device=self._device)
      return float("nan")
    per_batch = torch.stack(losses)
    if world > 1:  # sum over the ranks of rows_r * loss_r, divided by the global batch's rows
      torch.distributed.all_reduce(per_batch, op=torch.distributed.ReduceOp.SUM, group=self._group)
      per_batch = per_batch / torch.tensor(global_rows, dtype=per_batch.dtype, device=self._device)
    self.last_epoch_losses = per_batch
    return float(per_batch.mean())

  def evaluate_epoch(self, data, batch_size: int, *, generator: Optional[torch.Generator] = None,
                     shuffle: bool = False) -> float:
    """The reference's `evaluate_epoch` (dim/train.py:253-267, cil/train.py:221-235): `evaluate_step` per batch of
    `batch_size` rows (in order, or with `shuffle` in the order of `torch.randperm(len(data), generator=generator)`,
    kept in `self.last_permutation`) and the mean of the per-batch means, as a float.  Evaluation uses the running
    statistics, so every row's loss is independent of the rest of its batch: a batch larger than `max_batch` (the
    reference validates with 5x the training batch) runs in chunks of `max_batch` rows recombined as the row-weighted
    mean of the chunk means.  Every rank evaluates all of `data`."""
    if batch_size < 1:
      raise ValueError("batch_size=%d < 1" % batch_size)
    T = self._epoch_horizon()
    n = len(data)
    if shuffle:
      order = torch.randperm(n, device=self._device, generator=generator)
      self.last_permutation = order
    else:
      order = torch.arange(n, device=self._device)
    means = []
    for g0 in range(0, n, batch_size):
      rows = min(batch_size, n - g0)
      total = None
      for c0 in range(0, rows, self._max_batch):
        m = min(self._max_batch, rows - c0)
        loss = self.evaluate_step(data.batch(order[g0 + c0:g0 + c0 + m], T, mode=self._epoch_mode)) * m
        total = loss if total is None else total + loss
      means.append(total / rows)
    self.last_epoch_losses = torch.stack(means) if means else torch.zeros(0, device=self._device)
    return float(self.last_epoch_losses.mean()) if means else float("nan")

  # ---- views of the packed vectors in the reference's state_dict terms ----
  def _unpack(self, vector: torch.Tensor):
    out, pos = {}, 0
    for key, shape in self._packed_spec():
      n = int(np.prod(shape)) if len(shape) else 1
      out[key] = vector[pos:pos + n].view(*shape)
      pos += n
    return out

  def named_gradients(self):
    """`{state_dict key: gradient view}` (running-statistic keys hold zeros)."""
    return self._unpack(self.grads)

  def state_dict(self):
    """The trained weights as a reference-compatible `state_dict` (device tensors; `num_batches_tracked` counters are
    the number of train-mode forward passes, like nn.BatchNorm2d keeps them)."""
    sd = self._unpack(self.params)
    full = {}
    for key, _ in type(self)._state_dict_spec(self._C):
      if key.endswith("num_batches_tracked"):
        full[key] = torch.tensor(self.num_batches_tracked, dtype=torch.long)
      else:
        full[key] = sd[key].detach().clone()
    return full

  def sync_to_model(self):
    """Writes the trained weights into the wrapped model (its inference handle and every agent holding the model
    re-upload on their next call)."""
    self._model.load_state_dict({k: v.to(self._model.device) for k, v in self.state_dict().items()}, strict=True)
    return self._model

  def close(self) -> None:
    if self._h:
      self._lib.rip_train_destroy(self._h)
      self._h = ctypes.c_void_p(0)

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass


class DIMTrainer(_PackedTrainer):
  """One model, one device; owns the packed parameter / gradient / Adam-moment tensors and the HIP workspace.

  `deterministic=True` switches the deterministic mode on (`rip_train_set_option`): `backward`,
  `train_step`, `evaluate_step`, `train_epoch` and `evaluate_epoch` then produce the same bits on every run, in every
  trainer and every process, for the same inputs, the same state (parameters, Adam moments, step count), the same batch
  size, an identically seeded `generator` and the same device model.  This holds at world size 1 or with `group=None`;
  with a `group` the all-reduce's order belongs to the backend and is not covered.  Nothing is promised across batch
  sizes, world sizes or device models, and the mode's results equal the default's to fp32 rounding, not bit for bit.
  The target noise and the dropout mask of `train_step` come from torch's default device generator unless passed in
  (`y=`, `dropout_mask=`): seed it, or pass them, to repeat a single step."""

  _state_dict_spec = staticmethod(arch.state_dict_spec)

  def __init__(self, model: ImitativeModel, lr: float = 1e-3, weight_decay: float = 0.0, noise_level: float = 1e-2,
               max_batch: int = 512, device: Optional[torch.device] = None, betas=(0.9, 0.999), eps: float = 1e-8,
               group=None, deterministic: bool = False) -> None:
    self._noise = float(noise_level)
    super().__init__(model, lr, weight_decay, max_batch, device, betas, eps, group, deterministic)

  def _create(self) -> int:
    _lib.check(self._lib.rip_train_create(ctypes.byref(self._h), self._C, self._max_batch, self._device.index))
    return int(self._lib.rip_train_numel(self._C))

  def _packed_weights(self, model) -> np.ndarray:
    return model.packed_weights()

  # ---- the reference's train_step, in its two halves ----
  def backward(self, batch: Mapping[str, torch.Tensor], *, y: Optional[torch.Tensor] = None,
               dropout_mask: Optional[torch.Tensor] = None, train: bool = True, gradients: bool = True) -> torch.Tensor:
    """train.py:181-204: perturbs the target, runs the forward pass in train mode and back-propagates
    `-mean(log_prob - logabsdet)`; gradients land in `self.grads`.  Returns the loss (device scalar).
    `train=False`: running statistics, no dropout, no perturbation ("frozen" BatchNorm); `gradients=False`: forward
    only — loss and `self.z`, `self.grads` is left alone (`evaluate_step`)."""
    vis = self._visual(batch)
    B = vis.shape[0]
    vec = torch.cat([batch["velocity"].reshape(B, 3), batch["is_at_traffic_light"].reshape(B, 1),
                     batch["traffic_light_state"].reshape(B, 1)], dim=-1).to(torch.float32).contiguous()
    target = batch["player_future"][..., :2].to(torch.float32)
    _lib.expect_shape(target, (B, arch.T, 2), "player_future[..., :2]")
    if y is None:
      y = torch.normal(mean=target, std=float(self._noise)) if train else target  # train.py:184-189 (one launch)
    y = y.to(self._device, torch.float32).contiguous()
    dropout_mask = self._dropout_mask(B, train, dropout_mask)
    self.z = torch.empty(B, arch.HIDDEN_SIZE, device=self._device)
    self._last_batch = B
    _lib.check(self._lib.rip_train_forward_backward(
        self._h, _lib.ptr(self.params), _lib.ptr(self.grads if gradients else None), _lib.ptr(vis), _lib.ptr(vec), _lib.ptr(y),
        _lib.ptr(dropout_mask), B, int(train), _lib.ptr(self._loss.view(1)), _lib.ptr(self.z),
        _lib.current_stream(self._device)))
    if train:
      self.num_batches_tracked += 1
    return self._loss.clone()

  def _epoch_horizon(self) -> int:
    return arch.T

  def _target_noise(self, target, rows, a, b, generator):
    """train.py:184-189 for the epoch loop: N(0, noise_level^2) drawn for the whole global batch, this rank's slice
    added to its target."""
    noise = torch.empty((rows,) + tuple(target.shape[1:]), device=self._device).normal_(0.0, self._noise, generator=generator)
    return target + noise[a:b]

  def train_step(self, batch: Mapping[str, torch.Tensor], *, y: Optional[torch.Tensor] = None,
                 dropout_mask: Optional[torch.Tensor] = None, clip: bool = False) -> torch.Tensor:
    """train.py:175-213."""
    loss = self.backward(batch, y=y, dropout_mask=dropout_mask)
    self.apply(clip=clip)
    return loss

  def evaluate_step(self, batch: Mapping[str, torch.Tensor]) -> torch.Tensor:
    """train.py:229-249 (model.eval(): running statistics, no dropout, the unperturbed target)."""
    return self.backward(batch, train=False, gradients=False)

  def sync_to_model(self) -> ImitativeModel:
    """Writes the trained weights into the wrapped `ImitativeModel` (its inference handle and every agent holding
    the model re-upload on their next call)."""
    return super().sync_to_model()


  def publish(self, agent, k: int) -> None:
    """`agent.load_member(k, self)`: hands the current parameters to member `k` of a live `RIPAgent` on the device,
    behind the steps already issued on the current stream.  The wrapped model is not touched (`sync_to_model`)."""
    agent.load_member(k, self)


class CILTrainer(_PackedTrainer):
  """The behavioural-cloning step of oatomobile/baselines/torch/cil/train.py on one `BehaviouralModel`, one device:

      trainer = CILTrainer(model, lr=1e-3, weight_decay=0.0)   # optim.Adam(params, lr, weight_decay) (train.py:113-118)
      loss = trainer.train_step(batch, clip=False)              # train_step (train.py:168-190)
      loss = trainer.evaluate_step(batch)                       # evaluate_step (train.py:208-219)
      trainer.sync_to_model()                                   # the weights back into `model` (and its CILAgent)

  `batch` is what `BehaviouralModel.transform` produces (cil/model.py:129-170), on the device: `visual_features
  [B,C,100,100]`, `velocity [B,3]`, `is_at_traffic_light [B,1]`, `traffic_light_state [B,1]`, `mode [B,1]` and
  `player_future [B,T,>=2]`, T = `model._output_shape[0]` (the reference trains with T = 4).  Loss:
  `mean_b sum_{t,d} |predictions - player_future[..., :2]|` (nn.L1Loss(reduction="none") summed over [-2, -1]).
  Train mode: BatchNorm batch statistics (running statistics updated), Dropout(0.2) before the classifier — the only
  random draw (there is no target perturbation); `dropout_mask=` replays one.

  `deterministic=True` switches the deterministic mode on (`rip_train_set_option`): `backward`,
  `train_step`, `evaluate_step`, `train_epoch` and `evaluate_epoch` then produce the same bits on every run, in every
  trainer and every process, for the same inputs, the same state (parameters, Adam moments, step count), the same batch
  size, an identically seeded `generator` and the same device model.  This holds at world size 1 or with `group=None`;
  with a `group` the all-reduce's order belongs to the backend and is not covered.  Nothing is promised across batch
  sizes, world sizes or device models, and the mode's results equal the default's to fp32 rounding, not bit for bit."""

  _state_dict_spec = staticmethod(arch.cil_state_dict_spec)

  def __init__(self, model: BehaviouralModel, lr: float = 1e-3, weight_decay: float = 0.0, max_batch: int = 512,
               device: Optional[torch.device] = None, betas=(0.9, 0.999), eps: float = 1e-8, group=None,
               deterministic: bool = False) -> None:
    self._T = int(model._output_shape[0])
    super().__init__(model, lr, weight_decay, max_batch, device, betas, eps, group, deterministic)
    self.predictions = None

  _epoch_mode = True

  def _epoch_horizon(self) -> int:
    return self._T

  def _create(self) -> int:
    _lib.check(self._lib.rip_cil_train_create(ctypes.byref(self._h), self._C, self._T, self._max_batch,
                                              self._device.index))
    return int(self._lib.rip_cil_train_numel(self._C))

  def backward(self, batch: Mapping[str, torch.Tensor], *, dropout_mask: Optional[torch.Tensor] = None,
               train: bool = True, gradients: bool = True) -> torch.Tensor:
    """cil/train.py:176-183: forward in train mode, the L1 loss and its backward; gradients land in `self.grads`, the
    predictions [B,T,2] in `self.predictions`.  Returns the loss (device scalar).  `train=False`: running statistics,
    no dropout; `gradients=False`: forward only (`evaluate_step`), `self.grads` is left alone."""
    for key in ("visual_features", "velocity", "is_at_traffic_light", "traffic_light_state", "mode", "player_future"):
      if key not in batch:
        raise ValueError("Missing `%s` in the batch." % key)
    vis = self._visual(batch)
    B = vis.shape[0]
    vec = torch.cat([batch["velocity"].reshape(B, 3), batch["is_at_traffic_light"].reshape(B, 1),
                     batch["traffic_light_state"].reshape(B, 1), batch["mode"].reshape(B, 1)],
                    dim=-1).to(self._device, torch.float32).contiguous()  # cil/model.py:88-98
    target = batch["player_future"][..., :2].to(self._device, torch.float32).contiguous()
    _lib.expect_shape(target, (B, self._T, 2), "player_future[..., :2]")
    dropout_mask = self._dropout_mask(B, train, dropout_mask)
    self.predictions = torch.empty(B, self._T, 2, device=self._device)
    self._last_batch = B
    _lib.check(self._lib.rip_cil_train_forward_backward(
        self._h, _lib.ptr(self.params), _lib.ptr(self.grads if gradients else None), _lib.ptr(vis), _lib.ptr(vec),
        _lib.ptr(target), _lib.ptr(dropout_mask), B, int(train), _lib.ptr(self._loss.view(1)),
        _lib.ptr(self.predictions), _lib.current_stream(self._device)))
    if train:
      self.num_batches_tracked += 1
    return self._loss.clone()

  def train_step(self, batch: Mapping[str, torch.Tensor], *, dropout_mask: Optional[torch.Tensor] = None,
                 clip: bool = False) -> torch.Tensor:
    """cil/train.py:168-190: zero_grad, forward, L1 loss, backward, [clip_grad_norm(1.0)], Adam step."""
    loss = self.backward(batch, dropout_mask=dropout_mask)
    self.apply(clip=clip)
    return loss

  def evaluate_step(self, batch: Mapping[str, torch.Tensor]) -> torch.Tensor:
    """cil/train.py:208-219 (model.eval(): running statistics, no dropout); predictions in `self.predictions`."""
    return self.backward(batch, train=False, gradients=False)

  def sync_to_model(self) -> BehaviouralModel:
    """Writes the trained weights into the wrapped `BehaviouralModel`: its next `forward` (and every `CILAgent`
    holding it) runs on them."""
    return super().sync_to_model()


class HeadTrainer:
  """The density heads of ALL members of a `RIPAgent`'s ensemble trained on cached encoder features, one step for the K
  members in four launches whatever K and the batch (`rip_head_forward_backward` of include/rip_head.h: forward /
  backward, weight gradients, losses; then `rip_train_adam` on the flattened heads):

      cache = replay.FeatureCache.build(agent, data, 128)        # feat [K,n,128] once, encoders frozen
      trainer = HeadTrainer(agent, lr=1e-3)
      losses = trainer.train_epoch(cache, 128, generator=g)      # [K] per-member epoch losses
      trainer.publish(agent)                                     # the new weights into the live agent, on the device

  The head is `_merger` and `_decoder` (32 164 of the 2.4 M parameters, the tail of `arch.packed_spec()`); the encoder
  is frozen in eval mode, so its output per (member, observation) is a constant, there is no BatchNorm and no dropout,
  and the loss of a member is the reference's `-mean(log_prob - logabsdet)` (dim/train.py:198-204) on targets perturbed
  with N(0, noise_level^2) noise (train.py:184-189).  The step is deterministic by construction (no float atomics; sums
  over the rows in an order fixed by the batch size alone) and member k's results do not depend on K.

  State, all on the agent's device: `params` [K, P_head] (contiguous, what Adam steps), `grads`, `exp_avg`,
  `exp_avg_sq` of that shape, `step_count`, and `full` [K, packed_numel]: each member's whole packed vector, its
  encoder part as the agent's models had it at construction.  `params` is a tensor of its own, not a view of `full`
  (one Adam launch needs the K heads contiguous); `publish`, `state_dict` and `sync_to_models` copy it into `full`'s
  tail first.  There is no CPU path."""

  def __init__(self, agent, lr: float = 1e-3, weight_decay: float = 0.0, noise_level: float = 1e-2, max_batch: int = 512,
               betas=(0.9, 0.999), eps: float = 1e-8) -> None:
    if not torch.cuda.is_available():
      raise RuntimeError("oatomobile_amd.HeadTrainer needs a ROCm device; there is no CPU path.")
    if max_batch < 1:
      raise ValueError("max_batch=%d must be >= 1" % max_batch)
    self._lib = _lib.load()
    self._device = agent._device
    self._models = list(agent._models)
    self._C = agent._in_channels
    self.K = len(self._models)
    self.P = int(self._lib.rip_head_numel())
    spec = arch.packed_spec(self._C)
    self._head_spec = [(k, s) for k, s in spec if not k.startswith("_encoder.")]
    if sum(int(np.prod(s)) for _, s in self._head_spec) != self.P or spec[-len(self._head_spec):] != self._head_spec:
      raise RuntimeError("head layout mismatch: library %d floats, arch.packed_spec tail %d" %
                         (self.P, sum(int(np.prod(s)) for _, s in self._head_spec)))
    self._lr, self._wd, self._noise = float(lr), float(weight_decay), float(noise_level)
    self._betas, self._eps = (float(betas[0]), float(betas[1])), float(eps)
    self._max_batch = int(max_batch)
    self.full = torch.from_numpy(np.stack([m.packed_weights() for m in self._models])).to(self._device)
    self.params = self.full[:, -self.P:].clone()
    self.grads = torch.zeros_like(self.params)
    self.exp_avg = torch.zeros_like(self.params)
    self.exp_avg_sq = torch.zeros_like(self.params)
    self.step_count = 0
    self._workspace = torch.empty(int(self._lib.rip_head_workspace_bytes(self.K, self._max_batch)), dtype=torch.uint8,
                                  device=self._device)
    self.q_rows = self.z = None

  # ---- one step ----
  def _check(self, feat, vec, target, y, rows, noise):
    name = "HeadTrainer"
    for what, t in (("feat", feat), ("vec", vec), ("target", target), ("y", y), ("rows", rows), ("noise", noise)):
      if t is None:
        continue
      if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self._device:
        raise RuntimeError("%s: `%s` must be a tensor on %s (got %s) — no CPU path" %
                           (name, what, self._device, getattr(t, "device", type(t))))
    if feat.dim() != 3 or feat.shape[0] != self.K:
      raise ValueError("%s: feat must have shape [K=%d,n,%d], got %s" % (name, self.K, arch.NUM_FEATURES, tuple(feat.shape)))
    _lib.expect_shape(feat, (self.K, None, arch.NUM_FEATURES), "feat")
    n = int(feat.shape[1])
    _lib.expect_shape(vec, (n, arch.VECTOR_INPUTS), "vec")
    if rows is not None:
      if rows.dtype != torch.int64:
        raise ValueError("%s: rows must be int64, got %s" % (name, rows.dtype))
      _lib.expect_shape(rows, (self.K, None), "rows")
    B = n if rows is None else int(rows.shape[1])
    if B < 1 or B > self._max_batch:
      raise ValueError("%s: batch of %d rows outside [1, max_batch=%d]" % (name, B, self._max_batch))
    if (y is None) == (target is None):
      raise ValueError("%s: pass exactly one of `y` [K,B,4,2] and `target` [n,L,2]" % name)
    if y is not None:
      _lib.expect_shape(y, (self.K, B, arch.T, 2), "y")
      if noise is not None:
        raise ValueError("%s: `noise` goes with `target`; a dense `y` is taken as it is" % name)
    else:
      _lib.expect_shape(target, (n, None, 2), "target")
      if noise is not None:
        _lib.expect_shape(noise, (self.K, B, arch.T, 2), "noise")
    return n, B

  def backward(self, feat: torch.Tensor, vec: torch.Tensor, *, target: Optional[torch.Tensor] = None,
               y: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
               perturb: bool = True, gradients: bool = True) -> torch.Tensor:
    """Forward and backward of the K heads; the gradients land in `self.grads`, `q = log_prob - logabsdet` per row in
    `self.q_rows` [K,B] and the merger's output in `self.z` [K,B,64].  Returns the losses [K] (a fresh device tensor).

    `feat` [K,n,128] and `vec` [n,5] are the cached features and vector inputs of n observations; `rows` [K,B] int64
    picks each member's batch out of them (repeats allowed; None = all n rows in order for every member).  The target
    is either `y` [K,B,4,2], taken as it is, or `target` [n,L,2], the cached futures, gathered as
    `target[rows, 0::L // 4]` inside the kernel plus `noise` [K,B,4,2] (None with `perturb`: drawn here as
    N(0, noise_level^2) from torch's default device generator; `perturb=False`: none).  A row outside [0, n) gives that
    member a NaN loss and NaN gradients and leaves the other members alone.  `gradients=False`: forward only."""
    n, B = self._check(feat, vec, target, y, rows, noise)
    L = stride = 0
    if target is not None:
      L = int(target.shape[1])
      from oatomobile_amd.replay import downsample_stride
      stride = downsample_stride(L, arch.T)
      if noise is None and perturb and self._noise > 0.0:
        noise = torch.empty(self.K, B, arch.T, 2, device=self._device).normal_(0.0, self._noise)
    self.q_rows = torch.empty(self.K, B, device=self._device)
    self.z = torch.empty(self.K, B, arch.HIDDEN_SIZE, device=self._device)
    loss = torch.empty(self.K, device=self._device)
    _lib.check(self._lib.rip_head_forward_backward(
        _lib.ptr(self.params), _lib.ptr(self.grads if gradients else None), _lib.ptr(feat), _lib.ptr(vec), n,
        _lib.ptr(rows, torch.int64), _lib.ptr(y), _lib.ptr(target), L, stride, _lib.ptr(noise), self.K, B, self._max_batch,
        _lib.ptr(self._workspace, torch.uint8), _lib.ptr(self.q_rows), _lib.ptr(loss), _lib.ptr(self.z),
        _lib.current_stream(self._device)))
    return loss

  def apply(self) -> None:
    """`optimizer.step()` (torch.optim.Adam) for the K heads: one `rip_train_adam` on the flattened [K * P_head]."""
    self.step_count += 1
    _lib.check(self._lib.rip_train_adam(
        _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), None,
        self.params.numel(), self.step_count, self._lr, self._betas[0], self._betas[1], self._eps, self._wd,
        _lib.current_stream(self._device)))

  def train_step(self, feat, vec, *, target=None, y=None, rows=None, noise=None) -> torch.Tensor:
    """`backward` + `apply`; returns the losses [K] before the step."""
    loss = self.backward(feat, vec, target=target, y=y, rows=rows, noise=noise)
    self.apply()
    return loss

  def evaluate_step(self, feat, vec, *, target=None, y=None, rows=None) -> torch.Tensor:
    """Forward only on the unperturbed target: `q_rows` [K,B] (the losses are `-q_rows.mean(1)`)."""
    self.backward(feat, vec, target=target, y=y, rows=rows, perturb=False, gradients=False)
    return self.q_rows

  def train_epoch(self, features, batch_size: int, *, generator: Optional[torch.Generator] = None,
                  member_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One epoch over `features` (a `replay.FeatureCache`) with `DataLoader(shuffle=True, drop_last=False)` semantics,
    like `DIMTrainer.train_epoch`: `train_step` per batch, the last short batch included, and the mean of the
    per-batch losses per member, [K] on the device (no synchronisation).

    `member_rows` [K,m] int64 maps each member's epoch onto its own m cache rows (a bootstrap sample: repeats allowed);
    None = every member sees all n rows.  The random draws come from `generator` (a generator on this device; None =
    torch's default one) in this order: `torch.randperm(m)` once (kept in `self.last_permutation`; all members share
    it, over their own rows), then per batch the target noise N(0, noise_level^2) of shape [K, rows, 4, 2].  No batch
    is assembled: the kernel reads the cache rows through the index table."""
    if batch_size < 1 or batch_size > self._max_batch:
      raise ValueError("batch_size=%d outside [1, max_batch=%d]" % (batch_size, self._max_batch))
    if features.feat.shape[0] != self.K:
      raise ValueError("the feature cache holds %d members, the trainer %d" % (features.feat.shape[0], self.K))
    n = int(features.feat.shape[1])
    if member_rows is not None:
      if not isinstance(member_rows, torch.Tensor) or member_rows.dtype != torch.int64 or member_rows.device != self._device:
        raise ValueError("member_rows must be an int64 tensor on %s" % (self._device,))
      _lib.expect_shape(member_rows, (self.K, None), "member_rows")
    m = n if member_rows is None else int(member_rows.shape[1])
    perm = torch.randperm(m, device=self._device, generator=generator)
    self.last_permutation = perm
    losses = []
    for g0 in range(0, m, batch_size):
      idx = perm[g0:g0 + batch_size]
      rows = (idx.unsqueeze(0).expand(self.K, -1) if member_rows is None else member_rows[:, idx]).contiguous()
      noise = torch.empty(self.K, idx.numel(), arch.T, 2, device=self._device).normal_(0.0, self._noise, generator=generator)
      losses.append(self.train_step(features.feat, features.vec, target=features.future, rows=rows, noise=noise))
    self.last_epoch_losses = torch.stack(losses) if losses else torch.zeros(0, self.K, device=self._device)
    return self.last_epoch_losses.mean(0) if losses else torch.full((self.K,), float("nan"), device=self._device)

  # ---- the trained weights ----
  def _sync_full(self) -> None:
    self.full[:, -self.P:].copy_(self.params)

  def named_gradients(self, k: int):
    """`{state_dict key: gradient view}` of member `k`'s head."""
    return self._unpack(self.grads[k])

  def _unpack(self, vector: torch.Tensor):
    out, pos = {}, 0
    for key, shape in self._head_spec:
      cnt = int(np.prod(shape))
      out[key] = vector[pos:pos + cnt].view(*shape)
      pos += cnt
    return out

  def state_dict(self, k: int):
    """Member `k`'s weights as a reference-compatible `state_dict`: the encoder entries (and the BatchNorm counters) are
    the model's, the head entries the trainer's."""
    sd = {key: v.detach().clone() for key, v in self._models[k].state_dict().items()}
    for key, v in self._unpack(self.params[k]).items():
      sd[key] = v.detach().clone()
    return sd

  def publish(self, agent, members=None) -> None:
    """`agent.load_member(k, self.full[k])` for every member (or those of `members`): the trained heads into a live
    `RIPAgent` on the device, behind the steps already issued on the current stream.  The agent's captured
    one-observation pipelines stay unless a member's `split_wmax` flag changes (`RIPAgent.load_member`); the models are
    not touched (`sync_to_models`)."""
    self._sync_full()
    for k in (range(self.K) if members is None else members):
      agent.load_member(int(k), self.full[int(k)])

  def sync_to_models(self) -> None:
    """Writes the trained heads into the agent's `ImitativeModel`s (every agent holding them re-uploads on its next call)."""
    for k, m in enumerate(self._models):
      m.load_state_dict({key: v.to(m.device) for key, v in self.state_dict(k).items()}, strict=True)
