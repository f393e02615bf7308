"""ctypes binding of librip_hip.so (C ABI: include/rip_hip.h).

The product path has no CPU fallback: if the shared library is missing or does
not load, importing a symbol from here raises — run `python -c "import
__graft_entry__ as g; g.build()"` (hipcc, gfx950) first.
"""

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librip_hip.so")

# (name, restype, argtypes) — must list every symbol include/rip_hip.h declares.
SIGNATURES = [
    ("rip_abi_version", c_int, []),
    ("rip_last_error", c_char_p, []),
    ("rip_create", c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int]),
    ("rip_destroy", c_int, [c_void_p]),
    ("rip_load_model", c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    ("rip_load_model_device", c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    ("rip_peek_weights", c_int, [c_void_p, c_int, c_int, c_void_p, c_size_t, POINTER(c_size_t), c_void_p]),
    ("rip_model_flags", c_int, [c_void_p, c_int, POINTER(c_float), POINTER(c_int)]),
    ("rip_transform", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("rip_encode", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("rip_encode_tap", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    ("rip_encode_tap_k", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    ("rip_kernel_log", c_int, [c_void_p, c_char_p, c_size_t]),
    ("rip_encode_raw", c_int,
     [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("rip_encode_raw_u8", c_int,
     [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("rip_flow_forward", c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("rip_flow_inverse", c_int,
     [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("rip_goal_likelihood", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    ("rip_flow_vjp", c_int, [
        c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
        c_void_p, c_void_p
    ]),
    ("rip_flow_vjp_workspace_bytes", c_size_t, [c_int, c_int]),
    ("rip_goal_likelihood_vjp", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    ("rip_score", c_int,
     [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    ("rip_aggregate_scores", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("rip_lidar_bev", c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    ("rip_cil_decode", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ("rip_cil_blob_floats", c_int, []),
    ("rip_search", c_int, [
        c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p,
        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p
    ]),
    ("rip_mp_local", c_int,
     [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ("rip_mp_update", c_int, [
        c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p
    ]),
    ("rip_dim_forward", c_int,
     [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
      c_void_p]),
    ("rip_act", c_int, [
        c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
        c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p
    ]),
    ("rip_plan_stats", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("rip_act_stats", c_int, [
        c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
        c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p
    ]),
    ("rip_sample_normal", c_int, [c_uint64, c_uint64, c_int64, c_void_p, c_void_p]),
    ("rip_predict", c_int, [
        c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_uint64, c_int64, c_int, c_int, c_int, c_int,
        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p
    ]),
    ("rip_interpolate_plans", c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    ("rip_search_plan", c_int, [c_void_p, c_int, c_int, c_void_p, c_int]),
    ("rip_search_stats", c_int, [c_void_p, c_void_p, c_int]),
    ("rip_encoder_status", c_int, [c_void_p]),
    ("rip_trace_push", c_int, [c_char_p]),
    ("rip_trace_pop", c_int, []),
    ("rip_set_option", c_int, [c_void_p, c_int, c_int]),
    ("rip_num_models", c_int, [c_void_p]),
    ("rip_in_channels", c_int, [c_void_p]),
    ("rip_max_batch", c_int, [c_void_p]),
    ("rip_max_candidates", c_int, [c_void_p]),
    ("rip_train_numel", c_size_t, [c_int]),
    ("rip_train_create", c_int, [POINTER(c_void_p), c_int, c_int, c_int]),
    ("rip_train_destroy", c_int, [c_void_p]),
    ("rip_train_set_option", c_int, [c_void_p, c_int, c_int]),
    ("rip_train_trainable_mask", c_int, [c_void_p, c_void_p, c_size_t]),
    ("rip_train_forward_backward", c_int,
     [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("rip_train_peek", c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    ("rip_train_num_layers", c_int, [c_void_p]),
    ("rip_train_adam", c_int,
     [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_float, c_float, c_float, c_float, c_float,
      c_void_p]),
    ("rip_cil_train_numel", c_size_t, [c_int]),
    ("rip_cil_train_create", c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    ("rip_cil_train_forward_backward", c_int,
     [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("rip_gather_batch_u8", c_int, [
        c_void_p, c_void_p, c_void_p, c_int, ctypes.c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
        c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p
    ]),
    ("rip_hindsight_targets", c_int, [
        c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
        c_void_p, c_void_p, c_void_p, c_void_p
    ]),
    ("rip_code_bev_u8", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
]
ABI_VERSION = 4

# The extension header include/rip_head.h (the K-member head step on cached features): a table and a version of its
# own, resolved by the same `load()`; `SIGNATURES` and `ABI_VERSION` above are include/rip_hip.h's alone.
HEAD_SIGNATURES = [
    ("rip_head_abi_version", c_int, []),
    ("rip_head_numel", c_size_t, []),
    ("rip_head_workspace_bytes", c_size_t, [c_int, c_int]),
    ("rip_head_forward_backward", c_int, [
        c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int,
        c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p
    ]),
]
HEAD_ABI_VERSION = 1

ALGORITHMS = {"WCM": 0, "MA": 1, "BCM": 2}
ENC_DTYPES = {"fp32": 0, "bf16": 1}
OPT_SEARCH_KERNEL, OPT_ENCODER_FUSED, OPT_SEARCH_REGROUP, OPT_ENCODER_MEGA, OPT_DEBUG_ENCODER_FAULT = 0, 1, 2, 3, 4
OPT_ENCODER_VARIANT, OPT_KERNEL_LOG = 5, 6
ENC_VAR_IRB_ROUND3, ENC_VAR_FRONT_ROUND3, ENC_VAR_ROWS_F5_7, ENC_VAR_F17_LAYERWISE = 1, 2, 4, 8
ENC_VAR_FP32_LAYERWISE = 16  # fp32 encoder without the split-f16 tile blocks (encoder_split_tile.hip)
TRAIN_OPT_DETERMINISTIC = 1  # RIP_TRAIN_OPT_DETERMINISTIC of include/rip_hip.h (rip_train_set_option)
STAT_MEAN, STAT_VARIANCE, STAT_MIN, STAT_MAX, STAT_SLOTS = 0, 1, 2, 3, 4  # RIP_STAT_* of include/rip_hip.h
SPLIT_W_LIMIT = 200.0  # csrc/flow.h: a member with a flow weight of this magnitude keeps the fp32-MFMA search
SEARCH_KERNELS = {"auto": 0, "chain": 1, "phase": 3, "split": 4, "pair": 5}  # "pair": split-f16, paired workgroup shape forced


def search_kernel_id(name: str) -> int:
  """`search_kernel=` of the agents -> the value of `OPT_SEARCH_KERNEL`; a `ValueError` names the valid kernels
  (round 1's "mfma" kernel, option 2, was removed in round 5: the library answers RIP_EINVAL for it)."""
  try:
    return SEARCH_KERNELS[name]
  except KeyError:
    hint = " (\"mfma\", round 1's wave-per-model kernel, was removed: use \"split\" or \"phase\")" if name == "mfma" else ""
    raise ValueError("unknown search_kernel %r%s; valid: %s" % (name, hint, ", ".join(sorted(SEARCH_KERNELS)))) from None

_lib = None


RIP_OK, RIP_EINVAL, RIP_EHIP, RIP_ESTATE = 0, -1, -2, -3  # include/rip_hip.h


class RipError(RuntimeError):
  """A librip_hip.so entry point returned a negative code."""


def load() -> ctypes.CDLL:
  """Loads librip_hip.so once and types every entry point; raises if it is absent."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise ImportError(
        "oatomobile_amd: %s is missing — the HIP extension is not built "
        "(run `python -c \"import __graft_entry__ as g; g.build()\"`). There is no CPU fallback." % LIB_PATH)
  lib = ctypes.CDLL(LIB_PATH)
  for name, restype, argtypes in SIGNATURES + HEAD_SIGNATURES:
    fn = getattr(lib, name)  # AttributeError if the .so is stale
    fn.restype = restype
    fn.argtypes = argtypes
  _lib = lib
  return lib


def check(rc: int) -> None:
  if rc != 0:
    msg = load().rip_last_error()
    raise RipError("librip_hip error %d: %s" % (rc, msg.decode() if msg else "?"))


def ptr(t, dtype=None) -> c_void_p:
  """Device pointer of a contiguous fp32 (or `dtype`) HIP tensor, or NULL for None.  Raw pointers cross the C ABI
  unchecked on the other side, so dtype / residency / contiguity are enforced here."""
  if t is None:
    return c_void_p(0)
  import torch
  want = torch.float32 if dtype is None else dtype
  if not t.is_cuda:
    raise RuntimeError("oatomobile_amd: expected a ROCm device tensor, got one on %s (no CPU path)" % (t.device,))
  if t.dtype != want:
    raise ValueError("oatomobile_amd: expected a %s tensor, got %s" % (want, t.dtype))
  if not t.is_contiguous():
    raise ValueError("oatomobile_amd: expected a contiguous tensor (shape %s, strides %s)" % (tuple(t.shape), t.stride()))
  return c_void_p(t.data_ptr())


def current_stream(device=None) -> c_void_p:
  """torch's current stream ON `device` (a torch.device, an index or a tensor) — not on torch's current device:
  a handle on cuda:1 must never be handed cuda:0's stream."""
  import torch
  if device is not None and hasattr(device, "device"):
    device = device.device
  return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def expect_shape(t, shape, what: str) -> None:
  """ValueError unless `t.shape` matches `shape` (None = any extent)."""
  got = tuple(t.shape)
  if len(got) != len(shape) or any(w is not None and w != g for w, g in zip(shape, got)):
    raise ValueError("%s must have shape %s, got %s" % (what, "[" + ",".join("*" if w is None else str(w) for w in shape) + "]", got))


class Handle:
  """Owns one `rip_handle*` (K models on one device)."""

  def __init__(self, num_models: int, in_channels: int, max_batch: int, device_index: int,
               max_candidates: int = 1) -> None:
    self._lib = load()
    self._h = c_void_p(0)
    check(self._lib.rip_create(ctypes.byref(self._h), num_models, in_channels, max_batch, max_candidates, device_index))
    self.num_models, self.in_channels, self.max_batch, self.device_index = num_models, in_channels, max_batch, device_index
    self.max_candidates = max_candidates
    self.options = {}  # option -> the value last set through `set_option` (what a second handle over the same models mirrors)

  def stream(self) -> c_void_p:
    """torch's current stream on THIS handle's device."""
    return current_stream(self.device_index)

  @property
  def raw(self) -> c_void_p:
    return self._h

  def load_model(self, k: int, packed) -> None:
    import numpy as np
    packed = np.ascontiguousarray(packed, dtype=np.float32)
    check(self._lib.rip_load_model(self._h, k, packed.ctypes.data_as(c_void_p), packed.size))

  def load_model_device(self, k: int, packed) -> None:
    """`rip_load_model_device`: member `k` from a contiguous float32 tensor of `arch.packed_numel(C)` elements on the
    handle's device (the layout of `load_model`'s vector; `DIMTrainer.params` has it), on torch's current stream.  The
    fold and the re-layouts run on the device; the call waits for that stream once, for the member's flags."""
    import torch
    from oatomobile_amd import arch
    if not isinstance(packed, torch.Tensor):
      raise TypeError("load_model_device: expected a torch.Tensor, got %s" % type(packed).__name__)
    if not packed.is_cuda or packed.device.index != self.device_index:
      raise ValueError("load_model_device: the weights must be on cuda:%d, got %s" % (self.device_index, packed.device))
    want = arch.packed_numel(self.in_channels)
    if packed.dim() != 1 or packed.numel() != want:
      raise ValueError("load_model_device: expected %d packed floats (in_channels=%d), got shape %s" %
                       (want, self.in_channels, tuple(packed.shape)))
    check(self._lib.rip_load_model_device(self._h, k, ptr(packed), packed.numel(), self.stream()))

  def peek_weights(self, k: int, which: int):
    """`rip_peek_weights`: member `k`'s slice of weight buffer `which` (0..7, include/rip_hip.h) as a uint8 device tensor."""
    import torch
    n = c_size_t(0)
    check(self._lib.rip_peek_weights(self._h, k, which, None, 0, ctypes.byref(n), None))
    out = torch.empty(n.value, dtype=torch.uint8, device=torch.device("cuda", self.device_index))
    check(self._lib.rip_peek_weights(self._h, k, which, ptr(out, torch.uint8), n.value, None, self.stream()))
    return out

  def kernel_selection(self, k: int):
    """What of `model_flags` kernel selection reads: (the split-f16 search may take member `k`, the fp32 encoder's
    split-f16 blocks may).  A pipeline captured over the handle stays valid while this does not change."""
    wmax, ok = self.model_flags(k)
    return wmax < SPLIT_W_LIMIT, ok

  def model_flags(self, k: int):
    """`rip_model_flags` -> (split_wmax, enc_split_ok) of member `k`: what kernel selection reads."""
    wmax, ok = c_float(0.0), c_int(0)
    check(self._lib.rip_model_flags(self._h, k, ctypes.byref(wmax), ctypes.byref(ok)))
    return wmax.value, bool(ok.value)

  def set_option(self, option: int, value: int) -> None:
    check(self._lib.rip_set_option(self._h, option, value))
    self.options[option] = value

  def kernel_log(self) -> list:
    """The encoder kernels the handle's last encode / tap call launched (after `set_option(OPT_KERNEL_LOG, 1)`), one
    "kernel<template arguments> grid=(x,y,z) block=n" string per launch."""
    n = self._lib.rip_kernel_log(self._h, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    self._lib.rip_kernel_log(self._h, buf, n + 1)
    return [l for l in buf.value.decode().split("\n") if l]

  def close(self) -> None:
    if self._h:
      self._lib.rip_destroy(self._h)
      self._h = c_void_p(0)

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass


class trace_range:
  """`with trace_range("name"):` — a rocTX range through librip_hip.so's tracing hook (RIP_ROCTX=1; a no-op
  otherwise): the host-side counterpart of the ranges rip_encode / rip_search open."""

  def __init__(self, name: str) -> None:
    self._name = name.encode()

  def __enter__(self):
    load().rip_trace_push(self._name)
    return self

  def __exit__(self, *exc):
    load().rip_trace_pop()
    return False
