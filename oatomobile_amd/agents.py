"""Agents: `RIPAgent`, `DIMAgent` and the CARLA-free part of `SetPointAgent`.

Mirrors oatomobile/baselines/torch/rip/agent.py, .../dim/agent.py and
oatomobile/baselines/base.py.  `__call__(observation) -> [30, 3]` ego-frame
plan is the hot path (HIP); `act()` additionally needs CARLA's PID controller
and map, which the reference imports from the CARLA PythonAPI (base.py:71-77) —
with `environment=None` the agents run offline and `act()` returns the
setpoint/target-speed pair the PID would consume.
"""

import copy
import os
from typing import Any, Mapping, NamedTuple, Optional, Sequence

import numpy as np
import torch

from oatomobile_amd import _lib
from oatomobile_amd import arch
from oatomobile_amd import prediction
from oatomobile_amd.model import ImitativeModel

SIMULATOR_FPS = 20  # base.py:31
PLAN_ROWS = 30  # rows of the interpolated plan (rip/agent.py:141-151; RIP_PLAN_ROWS in include/rip_hip.h)


class PlanStats(NamedTuple):
  """Ensemble disagreement of trajectories (`rip_plan_stats`): `q` [K,B] or [K,B,M] = log q_k(y | x) of every member
  (the imitation prior, log_prob - logabsdet, without the goal term: it is the same for every member), and its `mean`,
  population `variance`, `min` and `max` over the K members, [B] or [B,M].  Device tensors from the batch entry points,
  numpy arrays in `RIPAgent.last_stats`."""
  q: Any
  mean: Any
  variance: Any
  min: Any
  max: Any


def _plan_stats(q, st) -> PlanStats:
  """(q [K,...], stats [...,4]) -> PlanStats of views."""
  return PlanStats(q, st[..., _lib.STAT_MEAN], st[..., _lib.STAT_VARIANCE], st[..., _lib.STAT_MIN], st[..., _lib.STAT_MAX])


def interpolate_plan(plan: np.ndarray, player_future_length: int = 40) -> np.ndarray:
  """rip/agent.py:141-151 == dim/agent.py:74-84: `[T,2]` -> `[(T-1)*inc, 3]` float64.
  Linear interpolation between knots every `inc = 40 // T` ticks (what
  `scipy.interpolate.interp1d` does there), evaluated at 0..knots[-1]-1, z = 0."""
  plan = np.asarray(plan)
  T = plan.shape[0]
  inc = player_future_length // T
  knots = np.arange(0, player_future_length, inc)[:T]  # time_index, rip/agent.py:145
  q = np.arange(0, int(knots[-1]))
  # scipy 1-D linear interpolation: the segment is found with a left-sided search (a query that sits on
  # a knot uses the segment ending there) and evaluated in slope form; (y_hi - y_lo) keeps the plan's
  # dtype (float32 from the device), the rest promotes to float64.
  hi = np.clip(np.searchsorted(knots, q), 1, T - 1)
  lo = hi - 1
  slope = (plan[hi] - plan[lo]) / (knots[hi] - knots[lo])[:, None]
  xy = slope * (q - knots[lo])[:, None] + plan[lo]
  return np.c_[xy, np.zeros((xy.shape[0], 1))].astype(np.float64)


def interpolate_plans(plans: torch.Tensor) -> torch.Tensor:
  """Batched R11 on the device (`rip_interpolate_plans`): plans [B,4,2] fp32 -> [B,30,3] float64, bit-identical to
  `interpolate_plan` row by row."""
  if not plans.is_cuda:
    raise RuntimeError("oatomobile_amd.interpolate_plans: expected a ROCm device tensor (no CPU path)")
  _lib.expect_shape(plans, (None, arch.T, 2), "plans")
  plans = plans.contiguous()
  out = torch.empty(plans.shape[0], PLAN_ROWS, 3, device=plans.device, dtype=torch.float64)
  with torch.cuda.device(plans.device):
    _lib.check(_lib.load().rip_interpolate_plans(_lib.ptr(plans), plans.shape[0], _lib.ptr(out, torch.float64),
                                                 _lib.current_stream(plans.device)))
  return out


def rot2mat(rotation: np.ndarray) -> np.ndarray:
  """utils/carla.py:642-649: `transforms3d.euler.euler2mat(roll, pitch, yaw).T` (static 'sxyz'),
  rotation given as (pitch, yaw, roll) in degrees like `carla.Rotation`."""
  pitch, yaw, roll = np.deg2rad(np.asarray(rotation, dtype=np.float64))
  ci, si = np.cos(roll), np.sin(roll)
  cj, sj = np.cos(pitch), np.sin(pitch)
  ck, sk = np.cos(yaw), np.sin(yaw)
  cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
  m = np.array([[cj * ck, sj * sc - cs, sj * cc + ss], [cj * sk, sj * ss + cc, sj * cs - sc], [-sj, cj * si, cj * ci]])
  return m.T


def world2local(*, current_location: np.ndarray, current_rotation: np.ndarray, world_locations: np.ndarray) -> np.ndarray:
  """utils/carla.py:652-674."""
  assert current_location.shape == (3,) and current_rotation.shape == (3,) and world_locations.ndim < 3
  world_locations = np.atleast_2d(world_locations)
  R = rot2mat(current_rotation)
  return np.squeeze(np.dot(R, (world_locations - current_location).T).T)


def local2world(*, current_location: np.ndarray, current_rotation: np.ndarray, local_locations: np.ndarray) -> np.ndarray:
  """utils/carla.py:677-700."""
  assert current_location.shape == (3,) and current_rotation.shape == (3,) and local_locations.ndim < 3
  local_locations = np.atleast_2d(local_locations)
  R_inv = np.linalg.inv(rot2mat(current_rotation))
  return np.dot(R_inv, local_locations.T).T + current_location


class SetPointAgent:
  """CARLA-free restatement of base.py:46-176: replan/buffer logic, ego->world
  transform and target speed.  With a CARLA `environment` the caller wires the
  returned setpoint into `VehiclePIDController.run_step` exactly as base.py:162-174."""

  def __init__(self, environment: Any = None, *, setpoint_index: int = 5, replan_every_steps: int = 1,
               lateral_control_dict: Optional[Mapping[str, Any]] = None,
               longitudinal_control_dict: Optional[Mapping[str, Any]] = None,
               fixed_delta_seconds_between_setpoints: Optional[float] = None) -> None:
    self._environment = environment
    self._setpoint_index = setpoint_index
    self._replan_every_steps = replan_every_steps
    self._lateral_control_dict = dict(lateral_control_dict or {"K_P": 1.95, "K_D": 0.01, "K_I": 1.4})
    self._longitudinal_control_dict = dict(longitudinal_control_dict or {"K_P": 1.0, "K_D": 0, "K_I": 1.0})
    self._fixed_delta_seconds_between_setpoints = fixed_delta_seconds_between_setpoints or 1.0 / SIMULATOR_FPS
    self._setpoints_buffer = None
    self._steps_counter = 0

  def __call__(self, observation, *args, **kwargs) -> np.ndarray:
    raise NotImplementedError

  def act(self, observation: Mapping[str, np.ndarray], *args, **kwargs):
    """base.py:116-176 up to the PID call: returns dict(setpoint [3] world frame = the location handed to
    `map.get_waypoint`, target_speed m/s (the PID gets it in km/h, :170-172), plan_world [T,3] = the setpoint
    buffer, predictions [T,3] = the buffer back in the ego frame, which the reference registers for rendering
    (:145-150))."""
    current_location = np.asarray(observation["location"], dtype=np.float64)
    current_rotation = np.asarray(observation["rotation"], dtype=np.float64)
    if self._setpoints_buffer is None or self._steps_counter % self._replan_every_steps == 0:
      plan_ego = self(copy.deepcopy(dict(observation)), *args, **kwargs)  # base.py:128
      self._setpoints_buffer = local2world(current_location=current_location, current_rotation=current_rotation,
                                           local_locations=plan_ego)
    else:
      self._setpoints_buffer = self._setpoints_buffer[1:]  # base.py:142
    predictions = world2local(current_location=current_location, current_rotation=current_rotation,
                              world_locations=self._setpoints_buffer)  # base.py:145-150
    self._steps_counter += 1
    target_speed = np.linalg.norm(np.diff(self._setpoints_buffer[:self._setpoint_index], axis=0),
                                  axis=1).mean() / self._fixed_delta_seconds_between_setpoints  # base.py:156-159
    if self._steps_counter <= 100:  # base.py:166-167
      target_speed = 20.0 / 3.6
    return dict(setpoint=self._setpoints_buffer[self._setpoint_index], target_speed=target_speed,
                plan_world=self._setpoints_buffer, predictions=predictions)

  def update(self, *args, **kwargs) -> None:  # core/agent.py:39-48
    return None


def _prepare_observation(observation: Mapping[str, Any], in_channels: int):
  """rip/agent.py:59-69 on the host (only the keys the model reads): float32 casts (any input dtype, like
  `.type(torch.float32)` there), goal[..., :2].  The BEV may have any H, W (the model resizes it to 100 x 100 like
  `F.interpolate`, torch/transforms.py:39-44); shapes that the kernels cannot take raise ValueError here."""
  lidar = np.ascontiguousarray(observation["lidar"], dtype=np.float32)
  if lidar.ndim != 3 or lidar.shape[-1] != in_channels or lidar.shape[0] < 1 or lidar.shape[1] < 1:
    raise ValueError("observation['lidar'] must be [H,W,%d], got %s" % (in_channels, lidar.shape))
  vec = np.concatenate([
      np.atleast_1d(np.asarray(observation["velocity"], dtype=np.float32)).reshape(3),
      np.atleast_1d(np.asarray(observation["is_at_traffic_light"], dtype=np.float32)).reshape(1),
      np.atleast_1d(np.asarray(observation["traffic_light_state"], dtype=np.float32)).reshape(1),
  ])
  goal = np.ascontiguousarray(np.asarray(observation["goal"], dtype=np.float32)[..., :2])
  if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] != 2:
    raise ValueError("observation['goal'] must be [G,>=2], got %s" % (np.shape(observation["goal"]),))
  return lidar, vec, goal


class RIPAgent(SetPointAgent):
  """The robust imitative planning agent (rip/agent.py:30-151) on one MI355X.

  Extra keyword arguments (defaults reproduce rip/agent.py:78-80,85-90):
    num_candidates: N latent starts searched in parallel (row 0 = zeros = the reference start,
      rows 1.. ~ N(0, I) from `seed`); each runs the reference recipe independently and the
      candidate with the lowest best-loss wins.  N = 1 is the reference algorithm.
    num_steps / lr / epsilon: hard-coded 10 / 0.1 / 1.0 in the reference.
    max_batch: observations per `plan_batch` call.
    encoder_dtype: "fp32" (parity mode, default) or "bf16" (BASELINE config 3: bf16 activations/weights in the
      MobileNetV2 encoder with fp32 accumulation; the flow and the search stay fp32).
    search_kernel: "auto" picks the MFMA-batched kernel once B*N >= 1280 (N % 16 == 0, any K <= 8), else the
      wave-per-chain kernel; both are the same algorithm.
    graph: `__call__` (one observation per call, the reference's usage) replays ONE captured hipGraph per call
      (H2D of the observation from pinned staging, transform, K encoders, search, D2H of the plan) instead of
      ~60 eager launches.  Same kernels, same results.
    stats: `__call__` also computes the ensemble disagreement of the plan it returns (`rip_act_stats`: one more kernel
      behind the search, its K + 4 floats in the same D2H copy as the plan) and leaves it in `last_stats`, a `PlanStats`
      of numpy arrays (q [K,1]; mean, variance, min, max [1]); None before the first call and with `stats=False`
      (default: the pipeline of a call is then unchanged).  The batch entry points take `return_stats=` per call.

  The agent uploads a snapshot of every model's weights; the snapshot is refreshed automatically when a model's
  `load_state_dict()` / `refresh()` ran since (the reference agent reads the live module weights).
  """

  def __init__(self, environment: Any = None, *, algorithm: str, models: Sequence[ImitativeModel],
               num_candidates: int = 1, num_steps: int = 10, lr: float = 1e-1, epsilon: float = 1.0, seed: int = 0,
               max_batch: int = 1, device: Optional[torch.device] = None, search_kernel: str = "auto",
               fused_encoder: Optional[int] = None, encoder_dtype: str = "fp32", graph: bool = True, stats: bool = False,
               **kwargs) -> None:
    assert algorithm in ("WCM", "MA", "BCM")  # rip/agent.py:43
    self._algorithm = algorithm
    super().__init__(environment=environment, **kwargs)
    if not torch.cuda.is_available():
      raise RuntimeError("oatomobile_amd.RIPAgent needs a ROCm device; there is no CPU path.")
    self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if self._device.index is None:
      self._device = torch.device("cuda", torch.cuda.current_device())
    self._models = [model.to(self._device) for model in models]  # rip/agent.py:50
    self._in_channels = self._models[0]._in_channels
    self._num_candidates, self._num_steps, self._lr, self._epsilon = int(num_candidates), int(num_steps), float(lr), float(epsilon)
    self._max_batch = int(max_batch)
    self._enc_dtype = _lib.ENC_DTYPES[encoder_dtype]
    self._twin_args = dict(algorithm=algorithm, num_candidates=num_candidates, num_steps=num_steps, lr=lr, epsilon=epsilon,
                           seed=seed, max_batch=max_batch, search_kernel=search_kernel, fused_encoder=fused_encoder,
                           encoder_dtype=encoder_dtype, graph=graph, stats=stats, **kwargs)
    self._stats = bool(stats)
    self.last_stats: Optional[PlanStats] = None
    self._handle = _lib.Handle(len(self._models), self._in_channels, self._max_batch, self._device.index,
                               max_candidates=self._num_candidates)
    self._versions = [None] * len(self._models)
    self._sync_weights()
    # "auto" | "chain" (one wave per candidate x model chain) | "phase" / "split" (16 candidates per wave on the matrix cores: fp32 MFMA / two-term f16)
    self._handle.set_option(_lib.OPT_SEARCH_KERNEL, _lib.search_kernel_id(search_kernel))
    if fused_encoder is None and "RIP_ENCODER_FUSED" in os.environ:
      fused_encoder = int(os.environ["RIP_ENCODER_FUSED"])
    if fused_encoder is not None:
      self._handle.set_option(_lib.OPT_ENCODER_FUSED, int(fused_encoder))
    if "RIP_ENCODER_MEGA" in os.environ:  # experimental one-launch fp32 encoder: 1 = batches of up to 4 observations, 0 / -1 never
      self._handle.set_option(_lib.OPT_ENCODER_MEGA, int(os.environ["RIP_ENCODER_MEGA"]))
    self._enc_status = _lib.load().rip_encoder_status
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((self._num_candidates, arch.T, 2)).astype(np.float32)
    x0[0] = 0.0  # base distribution mean (rip/agent.py:85)
    self._x0_rows = torch.from_numpy(x0).to(self._device)
    self._x0_cache = {}
    self._coded_z = {}  # batch -> (z, plan) scratch of plan_batch_coded
    self._eager_pending = False  # plan_batch* work launched on torch's current stream since the last __call__
    self._use_graph = bool(graph) and os.environ.get("RIP_NO_GRAPH", "0") != "1"
    self._online = {}  # (H, W, G) -> captured one-observation pipeline
    self._replay_twin = None  # `replay_twin()`: the second handle of `replay.replay_cache(streams=2)`

  def _sync_weights(self) -> bool:
    """Uploads the weights of every model whose version changed since the last upload."""
    changed = False
    for k, m in enumerate(self._models):
      if self._versions[k] != m._version:
        self._handle.load_model(k, m.packed_weights())
        self._versions[k] = m._version
        changed = True
    return changed

  def load_member(self, k: int, source) -> None:
    """Hands member `k` new weights ON THE DEVICE: `source` is a `DIMTrainer` (its `.params`) or a contiguous float32
    tensor of `arch.packed_numel(C)` elements on this agent's device, in the layout of `ImitativeModel.packed_weights()`.
    One `rip_load_model_device` per handle (this agent's, and the cached replay twin's if there is one) on torch's
    current stream, behind the training step that produced the weights: no copy to the host, no host fold, no
    device-wide synchronise.  The bytes that land in the handle equal those of `trainer.sync_to_model()` +
    `agent.refresh()`.

    The `ImitativeModel` objects are NOT touched: `agent.refresh()` or a model's `refresh()` / `load_state_dict()` goes
    back to THEIR weights, and `trainer.sync_to_model()` remains the way to bring trained weights into them.  The
    captured one-observation pipelines are kept (the weight buffers do not move) unless one of the member's two
    kernel-selection flags changed (`Handle.kernel_selection`): kernel selection is part of a capture, so they are dropped
    then and re-captured by the next call.  `ValueError` for a source on another device, with another channel count
    or length; `TypeError` for anything else, a `CILTrainer` included."""
    from oatomobile_amd import train as _train
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < len(self._models):
      raise ValueError("load_member: member index %r outside [0, %d)" % (k, len(self._models)))
    if isinstance(source, _train.DIMTrainer):
      if source._C != self._in_channels:
        raise ValueError("load_member: the trainer's model has %d BEV channels, this agent's %d" % (source._C, self._in_channels))
      packed = source.params
    elif isinstance(source, torch.Tensor):
      packed = source
    else:
      raise TypeError("load_member: `source` must be a DIMTrainer or a packed float32 device tensor, got %s%s" %
                      (type(source).__name__, " (CIL weights are another model's)" if isinstance(source, _train.CILTrainer) else ""))
    want = arch.packed_numel(self._in_channels)
    if packed.dim() != 1 or packed.numel() != want:
      raise ValueError("load_member: expected %d packed floats (in_channels=%d), got shape %s" %
                       (want, self._in_channels, tuple(packed.shape)))
    if packed.dtype != torch.float32 or not packed.is_contiguous():
      raise ValueError("load_member: the weights must be a contiguous float32 tensor, got %s%s" %
                       (packed.dtype, "" if packed.is_contiguous() else " (not contiguous)"))
    if not packed.is_cuda or packed.device != self._device:
      raise ValueError("load_member: the weights must be on %s, got %s" % (self._device, packed.device))
    k = int(k)
    if self._sync_weights():  # (members whose model changed go first, so that this load is not mistaken for theirs)
      self._online = {}
    before = self._handle.kernel_selection(k)
    self._handle.load_model_device(k, packed)
    self._versions[k] = self._models[k]._version
    self._eager_pending = True
    if self._handle.kernel_selection(k) != before:
      self._online = {}
    if self._replay_twin is not None:
      self._replay_twin.load_member(k, packed)

  def load_members(self, sources) -> None:
    """`load_member(k, sources[k])` for every member; `None` leaves a member as it is."""
    if len(sources) != len(self._models):
      raise ValueError("load_members: %d sources for %d members" % (len(sources), len(self._models)))
    for k, source in enumerate(sources):
      if source is not None:
        self.load_member(k, source)

  def twin(self) -> "RIPAgent":
    """A second agent over the SAME models and latent starts with a handle (weights snapshot + scratch) of its own: two
    handles on two streams let one batch's encoder run beside another batch's search (`replay.replay_cache(streams=2)`).
    A handle is not thread-safe and serialises its own calls, which is why overlap needs two (include/rip_hip.h)."""
    other = RIPAgent(None, models=self._models, device=self._device, **self._twin_args)
    other._x0_rows = self._x0_rows
    return other

  def replay_twin(self) -> "RIPAgent":
    """The cached `twin()` of `replay.replay_cache(streams=2)`, brought up to date: the options set on this agent's handle
    since it was built (`Handle.set_option`: kernel selection, encoder variant) are set on the twin's handle as well, so
    that both lanes launch the same kernels.  `refresh()` re-uploads the twin's weights with this agent's."""
    if self._replay_twin is None:
      self._replay_twin = self.twin()
    theirs = self._replay_twin._handle
    for option, value in self._handle.options.items():
      if option != _lib.OPT_DEBUG_ENCODER_FAULT and theirs.options.get(option) != value:  # (a one-shot test hook, no setting)
        theirs.set_option(option, value)
    return self._replay_twin

  def refresh(self) -> None:
    """Force a re-upload of all model weights (after in-place parameter edits without `model.refresh()`), the cached
    replay twin's snapshot included."""
    self._versions = [None] * len(self._models)
    self._sync_weights()
    if self._replay_twin is not None:
      self._replay_twin.refresh()

  def _x0(self, batch: int) -> torch.Tensor:
    if batch not in self._x0_cache:
      self._x0_cache[batch] = self._x0_rows.unsqueeze(0).expand(batch, -1, -1, -1).contiguous()
    return self._x0_cache[batch]

  def _check_batch(self, lidar: torch.Tensor, vec: torch.Tensor, goal: Optional[torch.Tensor], y: Optional[torch.Tensor] = None,
                   what: str = "plan_batch", pair_only: bool = False) -> None:
    """The C ABI takes raw pointers: dtype, device and shape are enforced here (ValueError / RuntimeError).  `goal`
    [B,G,2] (plan_batch) or `y` [B,4,2] / [B,M,4,2] (score_trajectories) is the third input; `pair_only` (predict_batch)
    checks lidar and vec alone."""
    third = ("goal", goal) if y is None else ("y", y)
    for name, t in (("lidar", lidar), ("vec", vec)) + (() if pair_only else (third,)):
      if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self._device:
        raise RuntimeError("%s: `%s` must be a tensor on %s (got %s)" %
                           (what, name, self._device, getattr(t, "device", type(t))))
      if t.dtype != torch.float32:
        raise ValueError("%s: `%s` must be float32, got %s" % (what, name, t.dtype))
    _lib.expect_shape(lidar, (None, None, None, self._in_channels), "lidar")
    b = lidar.shape[0]
    if b < 1 or b > self._max_batch or lidar.shape[1] < 1 or lidar.shape[2] < 1:
      raise ValueError("%s: lidar %s: batch must be in [1, max_batch=%d], H, W >= 1" %
                       (what, tuple(lidar.shape), self._max_batch))
    _lib.expect_shape(vec, (b, 5), "vec")
    if pair_only:  # predict_batch: its optional goal / target / noise are checked by _check_predict
      return
    if y is not None:
      _lib.expect_shape(y, (b, arch.T, 2) if y.dim() == 3 else (b, None, arch.T, 2), "y")
      if y.shape[1] < 1:
        raise ValueError("%s: y needs at least one trajectory per observation" % what)
      return
    _lib.expect_shape(goal, (b, None, 2), "goal")
    if goal.shape[1] < 1:
      raise ValueError("plan_batch: goal needs at least one waypoint")

  def _stats_out(self, b: int, m: Optional[int] = None):
    """Fresh (q [K,B] or [K,B,M], stats [B,4] or [B,M,4]) outputs of a statistics launch."""
    K, mid = len(self._models), (() if m is None else (m,))
    return (torch.empty((K, b) + mid, device=self._device, dtype=torch.float32),
            torch.empty((b,) + mid + (_lib.STAT_SLOTS,), device=self._device, dtype=torch.float32))

  def score_trajectories(self, lidar: torch.Tensor, vec: torch.Tensor, y: torch.Tensor) -> PlanStats:
    """Ensemble disagreement of GIVEN trajectories: lidar [B,H,W,C], vec [B,5] as `plan_batch`, y [B,4,2] or [B,M,4,2]
    (M trajectories per observation, e.g. the expert's future or a set of candidates) -> `PlanStats` of device tensors
    (q [K,B] / [K,B,M]; mean, variance, min, max [B] / [B,M]).  One `rip_encode_raw` for the K members, then one
    `rip_plan_stats` launch."""
    self._check_batch(lidar, vec, None, y=y, what="score_trajectories")
    if self._sync_weights():
      self._online = {}
    lidar, vec, y = lidar.contiguous(), vec.contiguous(), y.contiguous()
    b, K = lidar.shape[0], len(self._models)
    m = None if y.dim() == 3 else y.shape[1]
    z = torch.empty(K, b, 64, device=self._device, dtype=torch.float32)
    q, st = self._stats_out(b, m)
    lib, stream = _lib.load(), self._handle.stream()
    self._eager_pending = True
    _lib.check(lib.rip_encode_raw(self._handle.raw, _lib.ptr(lidar), 1, lidar.shape[1], lidar.shape[2], _lib.ptr(vec), b, 0, K,
                                  self._enc_dtype, _lib.ptr(z), stream))
    _lib.check(lib.rip_plan_stats(self._handle.raw, _lib.ptr(z), _lib.ptr(y), b, 1 if m is None else m, _lib.ptr(q),
                                  _lib.ptr(st), stream))
    return _plan_stats(q, st)

  def _features(self, visual: torch.Tensor, vec: torch.Tensor):
    b, K = visual.shape[0], len(self._models)
    feat = torch.empty(K, b, arch.NUM_FEATURES, device=self._device, dtype=torch.float32)
    z = torch.empty(K, b, arch.HIDDEN_SIZE, device=self._device, dtype=torch.float32)
    _lib.check(_lib.load().rip_encode(self._handle.raw, _lib.ptr(visual), _lib.ptr(vec), b, 0, K, self._enc_dtype, _lib.ptr(z),
                                      _lib.ptr(feat), self._handle.stream()))
    return feat, z

  def features_batch(self, lidar: torch.Tensor, vec: torch.Tensor):
    """The K members' encoder outputs on a batch: lidar [B,H,W,C], vec [B,5] as `plan_batch` -> `(feat [K,B,128],
    z [K,B,64])` — the classifier logits of each member's MobileNetV2 and the merger's output on them, from this agent's
    handle and `encoder_dtype`.  `rip_transform`, then one `rip_encode` with `feat_dev`.  What `train.HeadTrainer`
    trains on (`replay.FeatureCache` holds them for a whole cache); the encoder's kernel selection keys on B * K, so the
    bits are those of this batch composition."""
    self._check_batch(lidar, vec, None, what="features_batch", pair_only=True)
    if self._sync_weights():
      self._online = {}
    lidar, vec = lidar.contiguous(), vec.contiguous()
    b, H, W = lidar.shape[0], lidar.shape[1], lidar.shape[2]
    visual = torch.empty(b, self._in_channels, arch.INPUT_HW, arch.INPUT_HW, device=self._device, dtype=torch.float32)
    self._eager_pending = True
    with torch.cuda.device(self._device):  # rip_transform is stateless: it launches on the current device
      _lib.check(_lib.load().rip_transform(_lib.ptr(lidar), b, self._in_channels, H, W, 1, arch.INPUT_HW, _lib.ptr(visual),
                                           self._handle.stream()))
    return self._features(visual, vec)

  def features_batch_coded(self, codes: torch.Tensor, lut: torch.Tensor, vec: torch.Tensor):
    """`features_batch` on a CODED BEV (codes [B,H,W,C] uint8 into lut [256], as `plan_batch_coded`): the table is
    applied by `rip_gather_batch_u8` (rows 0 .. B - 1), whose image equals `rip_transform`'s on the decoded BEV bit for
    bit, then one `rip_encode` with `feat_dev`."""
    dev = self._device
    if not (isinstance(codes, torch.Tensor) and codes.is_cuda and codes.device == dev and codes.dtype == torch.uint8):
      raise ValueError("features_batch_coded: `codes` must be a uint8 tensor on %s" % (dev,))
    _lib.expect_shape(codes, (None, None, None, self._in_channels), "codes")
    b = codes.shape[0]
    if b < 1 or b > self._max_batch:
      raise ValueError("features_batch_coded: batch %d outside [1, max_batch=%d]" % (b, self._max_batch))
    _lib.expect_shape(lut, (256,), "lut")
    _lib.expect_shape(vec, (b, 5), "vec")
    if self._sync_weights():
      self._online = {}
    codes, vec = codes.contiguous(), vec.contiguous()
    visual = torch.empty(b, self._in_channels, arch.INPUT_HW, arch.INPUT_HW, device=dev, dtype=torch.float32)
    rows = torch.arange(b, device=dev, dtype=torch.int64)
    vec_out = torch.empty(b, 5, device=dev)
    future = torch.zeros(b, arch.T, 2, device=dev)  # the gather kernel's target slot: not used here
    self._eager_pending = True
    with torch.cuda.device(dev):
      _lib.check(_lib.load().rip_gather_batch_u8(
          _lib.ptr(codes, torch.uint8), _lib.ptr(lut), _lib.ptr(rows, torch.int64), b, b, self._in_channels, codes.shape[1],
          codes.shape[2], arch.INPUT_HW, _lib.ptr(vec), _lib.ptr(future), arch.T, arch.T, 1, None, _lib.ptr(visual),
          _lib.ptr(vec_out), _lib.ptr(torch.empty_like(future)), None, self._handle.stream()))
    return self._features(visual, vec)

  def plan_batch(self, lidar: torch.Tensor, vec: torch.Tensor, goal: torch.Tensor,
                 return_loss: bool = False, interpolate: bool = False, out: Optional[torch.Tensor] = None,
                 return_stats: bool = False):
    """Device-resident batched planning: lidar [B,H,W,C] (sensor layout; 200 x 200 from CARLA), vec [B,5],
    goal [B,G,2] with 1 <= G <= 64 (RIP_MAX_GOALS; `_lib.RipError` beyond it, nothing is launched) -> plans [B,4,2]
    (and best losses [B,N]).  One rip_act call (transform + K encoders + search).
    `interpolate=True` returns what `__call__` returns per observation instead — the [B,30,3] float64 plans of
    rip/agent.py:141-151 — computed by the candidate-selection kernel (R11 on the device, bit-identical to the
    reference's scipy arithmetic); `out` = a caller-owned result tensor to write into.  `return_stats=True` appends
    the ensemble disagreement of the returned plans, a `PlanStats` of device tensors (q [K,B]; mean, variance, min,
    max [B]), to the returned tuple: one more kernel behind the search (`rip_act_stats`), same plans and losses."""
    self._check_batch(lidar, vec, goal)
    if self._sync_weights():
      self._online = {}
    lidar, vec, goal = lidar.contiguous(), vec.contiguous(), goal.contiguous()
    b = lidar.shape[0]
    shape, dtype = ((b, PLAN_ROWS, 3), torch.float64) if interpolate else ((b, arch.T, 2), torch.float32)
    if out is None:
      out = torch.empty(shape, device=self._device, dtype=dtype)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != self._device or not out.is_contiguous():
      raise ValueError("plan_batch: `out` must be a contiguous %s tensor of shape %s on %s" % (dtype, shape, self._device))
    loss = torch.empty(b, self._num_candidates, device=self._device, dtype=torch.float32) if return_loss else None
    q, st = self._stats_out(b) if return_stats else (None, None)
    self._eager_pending = True
    if interpolate:
      self._launch_act(lidar, vec, goal, None, loss, out, q, st)
    else:
      self._launch_act(lidar, vec, goal, out, loss, None, q, st)
    if return_stats:
      return (out, loss, _plan_stats(q, st)) if return_loss else (out, _plan_stats(q, st))
    return (out, loss) if return_loss else out

  def plan_batch_coded(self, codes: torch.Tensor, lut: torch.Tensor, vec: torch.Tensor, goal: torch.Tensor,
                       interpolate: bool = False, out: Optional[torch.Tensor] = None, return_stats: bool = False):
    """`plan_batch` on a CODED BEV (the replay cache, `replay.PackedCache`): codes [B,H,W,C] uint8 indices into
    lut [256] float32 — the distinct float32 values of the BEV the cache was packed from — vec [B,5], goal [B,G,2].
    The table is applied inside the transform kernel (`rip_encode_raw_u8`), so the plans are bit-identical to
    `plan_batch` on the float32 BEV while a quarter of its bytes cross PCIe and HBM.  `return_stats=True` returns
    `(plans, PlanStats)` as `plan_batch` does (`rip_plan_stats` on the z and the plans of this call)."""
    dev = self._device
    if not (isinstance(codes, torch.Tensor) and codes.is_cuda and codes.device == dev and codes.dtype == torch.uint8):
      raise ValueError("plan_batch_coded: `codes` must be a uint8 tensor on %s" % (dev,))
    _lib.expect_shape(codes, (None, None, None, self._in_channels), "codes")
    b = codes.shape[0]
    if b < 1 or b > self._max_batch:
      raise ValueError("plan_batch_coded: batch %d outside [1, max_batch=%d]" % (b, self._max_batch))
    _lib.expect_shape(lut, (256,), "lut")
    _lib.expect_shape(vec, (b, 5), "vec")
    _lib.expect_shape(goal, (b, None, 2), "goal")
    if self._sync_weights():
      self._online = {}
    codes, vec, goal = codes.contiguous(), vec.contiguous(), goal.contiguous()
    shape, dtype = ((b, PLAN_ROWS, 3), torch.float64) if interpolate else ((b, arch.T, 2), torch.float32)
    if out is None:
      out = torch.empty(shape, device=dev, dtype=dtype)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != dev or not out.is_contiguous():
      raise ValueError("plan_batch_coded: `out` must be a contiguous %s tensor of shape %s on %s" % (dtype, shape, dev))
    K, N = len(self._models), self._num_candidates
    lib, st = _lib.load(), self._handle.stream()
    self._eager_pending = True
    z = self._coded_z.get(b)
    if z is None:
      z = self._coded_z[b] = (torch.empty(K, b, 64, device=dev), torch.empty(b, arch.T, 2, device=dev))
    z, plan4 = z
    _lib.check(lib.rip_encode_raw_u8(self._handle.raw, _lib.ptr(codes, torch.uint8), _lib.ptr(lut), codes.shape[1], codes.shape[2],
                                     _lib.ptr(vec), b, 0, K, self._enc_dtype, _lib.ptr(z), st))
    target = plan4 if interpolate else out
    _lib.check(lib.rip_search(self._handle.raw, _lib.ptr(z), _lib.ptr(goal), _lib.ptr(self._x0(b)), b, N, goal.shape[1],
                              _lib.ALGORITHMS[self._algorithm], self._num_steps, self._lr, self._epsilon, _lib.ptr(target),
                              None, None, None, None, None, None, st))
    if interpolate:
      _lib.check(lib.rip_interpolate_plans(_lib.ptr(plan4), b, _lib.ptr(out, torch.float64), st))
    if return_stats:
      q, stats = self._stats_out(b)
      _lib.check(lib.rip_plan_stats(self._handle.raw, _lib.ptr(z), _lib.ptr(target), b, 1, _lib.ptr(q), _lib.ptr(stats), st))
      return out, _plan_stats(q, stats)
    return out

  def _check_predict(self, what: str, b: int, num_samples, top_k, goal, target, noise, row0, seed):
    """The argument checks of `predict_batch*` behind the input checks (ValueError / RuntimeError before any launch)
    -> (S, top_k) as ints."""
    K = len(self._models)
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 1:
      raise ValueError("%s: num_samples must be an integer >= 1, got %r" % (what, num_samples))
    S = int(num_samples)
    M = K * S
    if M > prediction.MAX_CANDIDATES:
      raise ValueError("%s: K x num_samples = %d x %d = %d candidates per observation, at most %d" %
                       (what, K, S, M, prediction.MAX_CANDIDATES))
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= top_k <= min(M, prediction.MAX_TOP_K):
      raise ValueError("%s: top_k must be an integer in [1, min(M=%d, %d)], got %r" % (what, M, prediction.MAX_TOP_K, top_k))
    if int(row0) < 0 or not 0 <= int(seed) < 2**64:
      raise ValueError("%s: row0 >= 0 and 0 <= seed < 2**64, got row0=%r seed=%r" % (what, row0, seed))
    for name, t, shape in (("goal", goal, (b, None, 2)), ("target", target, (b, arch.T, 2)),
                           ("noise", noise, (b, K, S, arch.T, 2))):
      if t is None:
        continue
      if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self._device:
        raise RuntimeError("%s: `%s` must be a tensor on %s (got %s)" % (what, name, self._device, getattr(t, "device", type(t))))
      if t.dtype != torch.float32:
        raise ValueError("%s: `%s` must be float32, got %s" % (what, name, t.dtype))
      _lib.expect_shape(t, shape, name)
    if goal is not None and not 1 <= goal.shape[1] <= 64:
      raise ValueError("%s: goal needs 1 to 64 waypoints, got %d" % (what, goal.shape[1]))
    return S, int(top_k)

  def _predict(self, z, b: int, S: int, top_k: int, goal, target, noise, seed, row0, return_candidates: bool):
    """`rip_predict` on z [K,b,64] into fresh outputs -> `Prediction` (and the candidate set)."""
    K, dev = len(self._models), self._device
    M = K * S
    f32 = dict(device=dev, dtype=torch.float32)
    y_all, q = torch.empty((b, M, arch.T, 2), **f32), torch.empty((K, b, M), **f32)
    stats = torch.empty((b, M, _lib.STAT_SLOTS), **f32)
    loss_all = torch.empty((b, M), **f32) if return_candidates else None
    y_top, loss_top = torch.empty((b, top_k, arch.T, 2), **f32), torch.empty((b, top_k), **f32)
    index = torch.empty((b, top_k), device=dev, dtype=torch.int32)
    ade = torch.empty((b, top_k), **f32) if target is not None else None
    fde = torch.empty((b, top_k), **f32) if target is not None else None
    goal = None if goal is None else goal.contiguous()
    target = None if target is None else target.contiguous()
    noise = None if noise is None else noise.contiguous()
    _lib.check(_lib.load().rip_predict(
        self._handle.raw, _lib.ptr(z), _lib.ptr(goal), 0 if goal is None else goal.shape[1], self._epsilon, _lib.ptr(target),
        _lib.ptr(noise), int(seed), int(row0), b, S, top_k, _lib.ALGORITHMS[self._algorithm], _lib.ptr(y_all), _lib.ptr(q),
        _lib.ptr(stats), _lib.ptr(loss_all), _lib.ptr(y_top), _lib.ptr(loss_top), _lib.ptr(index, torch.int32), _lib.ptr(ade),
        _lib.ptr(fde), self._handle.stream()))
    pred = prediction.Prediction(y_top, loss_top, index, torch.div(index, S, rounding_mode="floor"), ade, fde)
    return (pred, y_all, q, loss_all) if return_candidates else pred

  def predict_batch(self, lidar: torch.Tensor, vec: torch.Tensor, *, num_samples: int, top_k: int = 1,
                    goal: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, seed: int = 0,
                    row0: int = 0, noise: Optional[torch.Tensor] = None, return_candidates: bool = False):
    """Open-loop ensemble prediction by sample-and-rank: lidar [B,H,W,C], vec [B,5] as `plan_batch`.  Every member j
    draws `num_samples` = S trajectories from its flow, all M = K S candidates (m = j S + s) are scored under all K
    members and aggregated with the agent's `algorithm` (minus the goal likelihood when `goal` [B,G,2] is given, with
    the agent's `epsilon`), and the `top_k` (<= min(M, 64)) lowest losses come back best-first as a `Prediction` of
    device tensors; with `target` [B,4,2] (the expert's future) it carries their displacement errors.  One
    `rip_encode_raw` for the K members, then one `rip_predict`.
    The latents come from the device's counter-based generator: sample ((row0 + b) K + j) S + s of `seed`
    (`prediction.philox_normal` on the host), so a data set walked in batches — `row0` = the index of the batch's first
    observation — draws the same samples whatever the batch size.  `noise` [B,K,S,4,2] replaces them.
    `return_candidates=True` appends `(y_all [B,M,4,2], q [K,B,M], loss_all [B,M])`: every candidate, the log q_k
    `rip_plan_stats` gives for it, and its loss."""
    self._check_batch(lidar, vec, None, what="predict_batch", pair_only=True)
    S, top_k = self._check_predict("predict_batch", lidar.shape[0], num_samples, top_k, goal, target, noise, row0, seed)
    if self._sync_weights():
      self._online = {}
    lidar, vec = lidar.contiguous(), vec.contiguous()
    b, K = lidar.shape[0], len(self._models)
    z = torch.empty(K, b, 64, device=self._device, dtype=torch.float32)
    self._eager_pending = True
    _lib.check(_lib.load().rip_encode_raw(self._handle.raw, _lib.ptr(lidar), 1, lidar.shape[1], lidar.shape[2], _lib.ptr(vec),
                                          b, 0, K, self._enc_dtype, _lib.ptr(z), self._handle.stream()))
    return self._predict(z, b, S, top_k, goal, target, noise, seed, row0, return_candidates)

  def predict_batch_coded(self, codes: torch.Tensor, lut: torch.Tensor, vec: torch.Tensor, *, num_samples: int,
                          top_k: int = 1, goal: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
                          seed: int = 0, row0: int = 0, noise: Optional[torch.Tensor] = None,
                          return_candidates: bool = False):
    """`predict_batch` on a CODED BEV (the replay cache): codes [B,H,W,C] uint8 indices into lut [256] float32, as
    `plan_batch_coded` takes them (`rip_encode_raw_u8`, then `rip_predict`): the bits of `predict_batch` on the float32
    BEV."""
    dev = self._device
    if not (isinstance(codes, torch.Tensor) and codes.is_cuda and codes.device == dev and codes.dtype == torch.uint8):
      raise ValueError("predict_batch_coded: `codes` must be a uint8 tensor on %s" % (dev,))
    _lib.expect_shape(codes, (None, None, None, self._in_channels), "codes")
    b = codes.shape[0]
    if b < 1 or b > self._max_batch:
      raise ValueError("predict_batch_coded: batch %d outside [1, max_batch=%d]" % (b, self._max_batch))
    _lib.expect_shape(lut, (256,), "lut")
    _lib.expect_shape(vec, (b, 5), "vec")
    S, top_k = self._check_predict("predict_batch_coded", b, num_samples, top_k, goal, target, noise, row0, seed)
    if self._sync_weights():
      self._online = {}
    codes, vec, K = codes.contiguous(), vec.contiguous(), len(self._models)
    z = torch.empty(K, b, 64, device=dev, dtype=torch.float32)
    self._eager_pending = True
    _lib.check(_lib.load().rip_encode_raw_u8(self._handle.raw, _lib.ptr(codes, torch.uint8), _lib.ptr(lut), codes.shape[1],
                                             codes.shape[2], _lib.ptr(vec), b, 0, K, self._enc_dtype, _lib.ptr(z),
                                             self._handle.stream()))
    return self._predict(z, b, S, top_k, goal, target, noise, seed, row0, return_candidates)

  def _launch_act(self, lidar, vec, goal, plan, loss, plan_interp=None, q=None, stats=None) -> None:
    b = lidar.shape[0]
    lib = _lib.load()
    if q is not None or stats is not None:
      _lib.check(lib.rip_act_stats(self._handle.raw, _lib.ptr(lidar), 1, lidar.shape[1], lidar.shape[2], _lib.ptr(vec),
                                   _lib.ptr(goal), _lib.ptr(self._x0(b)), b, self._num_candidates, goal.shape[1],
                                   _lib.ALGORITHMS[self._algorithm], self._num_steps, self._lr, self._epsilon,
                                   self._enc_dtype, _lib.ptr(plan), _lib.ptr(loss), _lib.ptr(plan_interp, torch.float64),
                                   _lib.ptr(q), _lib.ptr(stats), self._handle.stream()))
      return
    _lib.check(lib.rip_act(self._handle.raw, _lib.ptr(lidar), 1, lidar.shape[1], lidar.shape[2], _lib.ptr(vec),
                           _lib.ptr(goal), _lib.ptr(self._x0(b)), b, self._num_candidates, goal.shape[1],
                           _lib.ALGORITHMS[self._algorithm], self._num_steps, self._lr, self._epsilon, self._enc_dtype,
                           _lib.ptr(plan), _lib.ptr(loss), _lib.ptr(plan_interp, torch.float64), self._handle.stream()))

  # -- one observation per call (the reference's usage): pinned staging + one hipGraph replay ---------------
  def _online_state(self, H: int, W: int, G: int):
    key = (H, W, G)
    st = self._online.get(key)
    if st is not None:
      return st
    dev, C = self._device, self._in_channels
    # ONE pinned staging buffer and ONE device buffer hold (lidar | vec | goal): the observation travels as a single
    # H2D copy (a copy node costs ~5-10 us of the captured graph's timeline whatever its size)
    n_l = (H * W * C + 3) // 4 * 4
    n_g = (G * 2 + 3) // 4 * 4
    obs_h = torch.zeros(n_l + 8 + n_g, dtype=torch.float32).pin_memory()
    obs_d = torch.zeros(n_l + 8 + n_g, dtype=torch.float32, device=dev)

    def views(buf):
      return (buf[:H * W * C].view(1, H, W, C), buf[n_l:n_l + 5].view(1, 5), buf[n_l + 8:n_l + 8 + G * 2].view(1, G, 2))

    lidar_h, vec_h, goal_h = views(obs_h)
    lidar_d, vec_d, goal_d = views(obs_d)
    if self._stats:
      # (plan [1,30,3] float64 | stats [1,4] | q [K,1]) in ONE device buffer and ONE pinned buffer: the K + 4 floats of
      # the statistics ride in the plan's D2H copy node (720 bytes of plan keep the 16-byte statistics row aligned)
      K, nb, ns = len(self._models), PLAN_ROWS * 3 * 8, 4 * _lib.STAT_SLOTS

      def outs(buf):
        return (buf[:nb].view(torch.float64).view(1, PLAN_ROWS, 3), buf[nb + ns:].view(torch.float32).view(K, 1),
                buf[nb:nb + ns].view(torch.float32).view(1, _lib.STAT_SLOTS))

      out_h = torch.zeros(nb + 4 * (K + _lib.STAT_SLOTS), dtype=torch.uint8).pin_memory()
      out_d = torch.zeros(nb + 4 * (K + _lib.STAT_SLOTS), dtype=torch.uint8, device=dev)
      plan_h, q_h, stat_h = outs(out_h)
      plan_d, q_d, stat_d = outs(out_d)
    else:
      plan_h = out_h = torch.empty(1, PLAN_ROWS, 3, dtype=torch.float64).pin_memory()
      plan_d = out_d = torch.empty(1, PLAN_ROWS, 3, dtype=torch.float64, device=dev)
      q_h = stat_h = q_d = stat_d = None
    st = dict(
        obs_h=obs_h, obs_d=obs_d, lidar_h=lidar_h, vec_h=vec_h, goal_h=goal_h,
        plan_h=plan_h,
        lidar_d=lidar_d, vec_d=vec_d, goal_d=goal_d,
        plan_d=plan_d, out_h=out_h, out_d=out_d, q_h=q_h, stat_h=stat_h, q_d=q_d, stat_d=stat_d,
        stream=torch.cuda.Stream(device=dev), graph=None)
    st["lidar_np"], st["vec_np"], st["goal_np"] = st["lidar_h"].numpy(), st["vec_h"].numpy(), st["goal_h"].numpy()
    self._x0(1)

    def pipeline():
      st["obs_d"].copy_(st["obs_h"], non_blocking=True)
      self._launch_act(st["lidar_d"], st["vec_d"], st["goal_d"], None, None, st["plan_d"], st["q_d"], st["stat_d"])  # R2..R11
      st["out_h"].copy_(st["out_d"], non_blocking=True)  # rip/agent.py:139 (720 bytes: the interpolated plan)

    st["pipeline"] = pipeline
    if self._use_graph:
      try:
        with torch.cuda.device(dev):
          st["stream"].wait_stream(torch.cuda.current_stream(dev))
          with torch.cuda.stream(st["stream"]):
            pipeline()  # warm-up on the capture stream: one-time kernel attributes, handle stream hand-over
          st["stream"].synchronize()
          g = torch.cuda.CUDAGraph()
          with torch.cuda.graph(g, stream=st["stream"]):
            pipeline()
          st["graph"] = g
      except Exception as e:  # capture unsupported in this runtime: same kernels, launched eagerly
        import warnings
        warnings.warn("oatomobile_amd.RIPAgent: hipGraph capture failed (%r); using eager launches" % (e,))
        st["graph"] = None
        torch.cuda.synchronize(dev)
    self._online[key] = st
    return st

  def __call__(self, observation: Mapping[str, np.ndarray], _retry: bool = False) -> np.ndarray:
    """Returns the imitative-prior plan [30, 3] in ego coordinates (rip/agent.py:52-151)."""
    # rip/agent.py:59-69 straight into the pinned staging buffer (float32 casts happen in the assignments; shapes that
    # the kernels cannot take raise ValueError like `_prepare_observation`)
    lidar = observation["lidar"]
    goal = observation["goal"]
    if not isinstance(lidar, np.ndarray):
      lidar = np.asarray(lidar, dtype=np.float32)
    if not isinstance(goal, np.ndarray):
      goal = np.asarray(goal, dtype=np.float32)
    if getattr(lidar, "ndim", 0) != 3 or lidar.shape[-1] != self._in_channels or lidar.shape[0] < 1 or lidar.shape[1] < 1:
      raise ValueError("observation['lidar'] must be [H,W,%d], got %s" % (self._in_channels, np.shape(lidar)))
    if getattr(goal, "ndim", 0) != 2 or goal.shape[0] < 1 or goal.shape[1] < 2:
      raise ValueError("observation['goal'] must be [G,>=2], got %s" % (np.shape(goal),))
    if self._sync_weights():
      self._online = {}
    st = self._online_state(lidar.shape[0], lidar.shape[1], goal.shape[0])
    np.copyto(st["lidar_np"][0], lidar, casting="unsafe")
    vec = st["vec_np"][0]
    vec[:3] = np.reshape(observation["velocity"], 3)
    vec[3] = np.reshape(observation["is_at_traffic_light"], -1)[0]
    vec[4] = np.reshape(observation["traffic_light_state"], -1)[0]
    np.copyto(st["goal_np"][0], goal[:, :2], casting="unsafe")
    # ~45 us of every call are host time; the stream / device context managers of the generic path cost ~15 of them, so
    # the common case (the agent's device is current) skips them and only orders the replay behind eager work this
    # agent itself launched (`_eager_pending`; callers that drive the C ABI on the handle directly and then call the
    # agent synchronise themselves, like any two users of one stream-ordered scratch)
    stream = st["stream"]
    if st["graph"] is not None and torch.cuda.current_device() == self._device.index:
      prev = torch.cuda.current_stream(self._device)
      if self._eager_pending:
        stream.wait_stream(prev)  # plan_batch* work of this agent still in flight on the caller's stream
        self._eager_pending = False
      torch.cuda.set_stream(stream)
      try:
        st["graph"].replay()
      finally:
        torch.cuda.set_stream(prev)
      stream.synchronize()  # (polling stream.query() instead measured no faster: 457.7 vs 456.3 us p50)
    else:
      with torch.cuda.device(self._device):
        stream.wait_stream(torch.cuda.current_stream(self._device))  # earlier eager work on this handle
        with torch.cuda.stream(stream):
          if st["graph"] is not None:
            st["graph"].replay()
          else:
            st["pipeline"]()
        stream.synchronize()
      self._eager_pending = False
    if self._enc_status(self._handle.raw):
      # the one-launch encoder found its workgroups off their XCDs or a layer barrier timed out: this call's z is
      # invalid.  The handle has switched to the layer-wise launches (for good); drop the captured graphs and repeat
      # the call ONCE.  rip_encoder_status is one-shot, and the repeat is bounded here as well: a status raised a
      # second time is an error, not another retry.
      if _retry:
        raise RuntimeError("the encoder reported a failure again after falling back to the layer-wise launches")
      self._online = {}
      return self.__call__(observation, _retry=True)  # (refreshes `last_stats` as well)
    if self._stats:
      self.last_stats = _plan_stats(st["q_h"].numpy().copy(), st["stat_h"].numpy().copy())
    return st["plan_h"].numpy()[0].copy()  # [30, 3] float64: R11 ran in the selection kernel


class DIMAgent(SetPointAgent):
  """The deep imitative model agent (dim/agent.py:31-84): single-model mode search."""

  def __init__(self, environment: Any = None, *, model: ImitativeModel, device: Optional[torch.device] = None,
               **kwargs) -> None:
    super().__init__(environment=environment, **kwargs)
    if not torch.cuda.is_available():
      raise RuntimeError("oatomobile_amd.DIMAgent needs a ROCm device; there is no CPU path.")
    self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    self._model = model.to(self._device)

  def __call__(self, observation: Mapping[str, np.ndarray], **kwargs) -> np.ndarray:
    lidar, vec, goal = _prepare_observation(observation, self._model._in_channels)
    from oatomobile_amd.model import transform_visual
    lidar_d = torch.from_numpy(lidar).to(self._device).unsqueeze(0)
    vis = transform_visual(lidar_d, channels_last=True)
    vec_d = torch.from_numpy(vec).to(self._device).unsqueeze(0)
    plan = self._model(num_steps=kwargs.get("num_steps", 20), epsilon=kwargs.get("epsilon", 1.0),
                       lr=kwargs.get("lr", 5e-2), x0=kwargs.get("x0"), goal=torch.from_numpy(goal).to(self._device).unsqueeze(0),
                       visual_features=vis, velocity=vec_d[:, :3], is_at_traffic_light=vec_d[:, 3:4],
                       traffic_light_state=vec_d[:, 4:5]).cpu().numpy()[0]  # dim/agent.py:69-72
    return interpolate_plan(plan)
