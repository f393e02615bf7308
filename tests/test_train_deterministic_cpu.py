"""The deterministic training mode's surface, without a GPU: the header's declaration and constant against `_lib`, the
command-line flag, and the trainers' keyword."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_option_call_and_its_constant():
  from oatomobile_amd import _lib
  header = open(os.path.join(ROOT, "include", "rip_hip.h")).read()
  assert re.search(r"^int rip_train_set_option\(rip_trainer\* t, int option, int value\);", header, re.M)
  value = re.search(r"^#define RIP_TRAIN_OPT_DETERMINISTIC (\d+)$", header, re.M)
  assert value and int(value.group(1)) == _lib.TRAIN_OPT_DETERMINISTIC == 1
  sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}["rip_train_set_option"]
  assert sig == (_lib.c_int, [_lib.c_void_p, _lib.c_int, _lib.c_int])
  assert hasattr(_lib.load(), "rip_train_set_option")
  # the comment block of the training step states the guarantee and its limits
  block = header[header.index("rip_train_set_option(t, RIP_TRAIN_OPT_DETERMINISTIC, 1)"):header.index("typedef struct rip_trainer")]
  assert "GUARANTEED" in block and "NOT guaranteed" in block and "all-reduce" in block


def test_command_line_accepts_deterministic_and_defaults_to_off():
  from oatomobile_amd.baselines.torch import _train_main
  base = ["--dataset_dir", "d", "--output_dir", "o", "--num_epochs", "1"]
  for kind in ("dim", "cil"):
    assert _train_main.parse_args(kind, base).deterministic is False
    assert _train_main.parse_args(kind, base + ["--deterministic"]).deterministic is True


def test_trainers_take_the_keyword_and_expose_a_read_only_property():
  from oatomobile_amd import CILTrainer, DIMTrainer
  for cls in (DIMTrainer, CILTrainer):
    assert inspect.signature(cls.__init__).parameters["deterministic"].default is False
    prop = inspect.getattr_static(cls, "deterministic")
    assert isinstance(prop, property) and prop.fset is None
    assert "deterministic=True" in cls.__doc__ and "all-reduce" in cls.__doc__
