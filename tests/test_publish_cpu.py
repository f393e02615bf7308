"""The device weight hand-off's host side, without a GPU: the three declarations of include/rip_hip.h against
`_lib.SIGNATURES` and the library, the argument checks that need no handle, and `RIPAgent.load_member`'s refusals.
(A handle cannot exist without a device: the checks that need one are in tests/test_publish.py.)"""

import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rip_load_model_device": 5, "rip_peek_weights": 7, "rip_model_flags": 4}


def test_header_bindings_and_library_agree():
  from oatomobile_amd import _lib
  header = open(os.path.join(ROOT, "include", "rip_hip.h")).read()
  sigs = {name: args for name, _, args in _lib.SIGNATURES}
  lib = _lib.load()
  for name, nargs in NEW.items():
    decl = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert decl is not None, name
    assert len(decl.group(1).split(",")) == nargs == len(sigs[name]), name
    assert hasattr(lib, name)
  assert len(set(re.findall(r"\b(rip_[a-z0-9_]+)\s*\(", header))) == len(_lib.SIGNATURES) == 61
  assert lib.rip_abi_version() == 4
  for method in ("load_model_device", "peek_weights", "model_flags"):
    assert callable(getattr(_lib.Handle, method))


def test_arguments_are_refused_before_any_launch():
  from oatomobile_amd import _lib
  lib = _lib.load()
  p = lambda v=256: _lib.c_void_p(v)  # never dereferenced: every call below is refused
  size = _lib.c_size_t(0)
  wmax, ok = _lib.c_float(0.0), _lib.c_int(0)
  for call, word in (
      (lambda: lib.rip_load_model_device(None, 0, p(), 10, None), "NULL"),
      (lambda: lib.rip_peek_weights(None, 0, 0, None, 0, _lib.ctypes.byref(size), None), "NULL"),
      (lambda: lib.rip_peek_weights(None, 0, 8, None, 0, _lib.ctypes.byref(size), None), "unknown weight buffer 8"),
      (lambda: lib.rip_peek_weights(None, 0, -1, None, 0, _lib.ctypes.byref(size), None), "unknown weight buffer -1"),
      (lambda: lib.rip_model_flags(None, 0, _lib.ctypes.byref(wmax), _lib.ctypes.byref(ok)), "NULL"),
  ):
    assert call() == _lib.RIP_EINVAL
    assert word in lib.rip_last_error().decode(), lib.rip_last_error()


def bare_agent(C=2, K=2):
  """A RIPAgent without a device: only what `load_member` reads before it touches the handle."""
  from oatomobile_amd import RIPAgent

  class Model:
    _version = 0

  agent = object.__new__(RIPAgent)
  agent._models, agent._in_channels, agent._device = [Model() for _ in range(K)], C, torch.device("cuda", 0)
  return agent


def test_load_member_refuses_what_it_cannot_load():
  from oatomobile_amd import CILTrainer, DIMTrainer, arch
  agent = bare_agent()
  n = arch.packed_numel(2)
  with pytest.raises(TypeError, match="CIL"):
    agent.load_member(1, object.__new__(CILTrainer))
  with pytest.raises(TypeError):
    agent.load_member(1, [0.0] * n)
  other = object.__new__(DIMTrainer)
  other._C = 3
  with pytest.raises(ValueError, match="3 BEV channels"):
    agent.load_member(1, other)
  with pytest.raises(ValueError, match="packed floats"):
    agent.load_member(1, torch.zeros(n - 1))
  with pytest.raises(ValueError, match="packed floats"):
    agent.load_member(1, torch.zeros(n + 1))
  with pytest.raises(ValueError, match="packed floats"):
    agent.load_member(1, torch.zeros(arch.packed_numel(3)))
  with pytest.raises(ValueError, match="float32"):
    agent.load_member(1, torch.zeros(n, dtype=torch.float64))
  with pytest.raises(ValueError, match="must be on cuda:0"):
    agent.load_member(1, torch.zeros(n))
  for k in (-1, 2, True, 0.5):
    with pytest.raises(ValueError, match="member index"):
      agent.load_member(k, torch.zeros(n))
  with pytest.raises(ValueError, match="sources"):
    agent.load_members([None])
  agent.load_members([None, None])  # nothing to do
