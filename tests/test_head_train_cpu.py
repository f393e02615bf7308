"""The head step's host side, without a GPU: the float64 restatement the GPU tests compare against (tests/head_ref.py)
checked against the oracle's full model, include/rip_head.h against `_lib.HEAD_SIGNATURES` and the library, the argument
refusals that precede any launch, the head's place in the packed layout, and two facts about the GPU tests' fixed inputs
that are established here: the ReLU-kink condition and the learning-curve margin.

Learning-curve margin (test_learning_curve_margin): over the learning test's 40 Adam steps on 64 rows, K = 2, the
float32 run of `head_ref` deviates from the float64 run by at most 1.52e-7 of the loss (largest |l32 - l64| / |l64| over
steps and members, measured; `head_ref.LEARNING_MARGIN` = 1.6e-7 covers it).  The GPU test's bound is ten times that constant:
two fp32 implementations that sum in different orders may each be that far from float64, and Adam compounds it."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oatomobile_amd import _lib, arch
from oatomobile_amd import weights as W
from tests import head_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_head_ref_matches_the_oracles_full_model():
  """`head_ref` (float64, features given) against `oracle.train_cpu.trainable_model(...).eval()` + `loss_and_grads`
  (fp32, the whole network) at B = 3, the features being that model's own eval-mode encoder output: the loss and every
  head gradient agree to 1e-4 of the tensor's largest magnitude (an fp32 autograd sum carries an absolute error
  proportional to its terms, so elements that cancel to nearly zero are held to the tensor's scale, not their own)."""
  from oracle import reference_cpu as O
  from oracle import train_cpu as TC
  from tests.helpers import synth_observation
  sd = W.synthetic_state_dict(211)
  model = TC.trainable_model(sd).eval()
  rng = np.random.default_rng(77)
  obs = [synth_observation(rng) for _ in range(3)]
  vis = O.transform_visual(torch.tensor(np.stack([o["lidar"] for o in obs])).permute(0, 3, 1, 2))
  vec = R.case_vec(rng, 3)
  y = R.case_targets(rng, 1, 3)[0]
  vt = torch.tensor(vec)
  loss, _ = TC.loss_and_grads(model, vis, vt[:, 0:3], vt[:, 3:4], vt[:, 4:5], torch.tensor(y), None)
  with torch.no_grad():
    feat = model._encoder(vis).numpy()
  ref = R.head_ref(R.head_model(W.pack_state_dict(sd)[-R.HEAD_NUMEL:]), feat, vec, y)
  assert abs(ref["loss"] - float(loss)) <= 1e-4 * abs(ref["loss"]), (ref["loss"], float(loss))
  named = dict(model.named_parameters())
  for key in R.HEAD_KEYS:
    got, want = named[key].grad.numpy().astype(np.float64), ref["grads"][key]
    assert got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 1e-4, (key, err)


def test_header_signatures_library_agree():
  """Every declaration of include/rip_head.h is bound in `_lib.HEAD_SIGNATURES` with the same argument count and is
  exported; the extension has its own version and leaves rip_hip.h's table alone."""
  header = open(os.path.join(ROOT, "include", "rip_head.h")).read()
  body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
  decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(rip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body)}
  sigs = {name: args for name, _, args in _lib.HEAD_SIGNATURES}
  assert set(decls) == set(sigs) and len(sigs) == len(_lib.HEAD_SIGNATURES)
  lib = _lib.load()
  for name, args in decls.items():
    n = 0 if args.strip() in ("", "void") else len(args.split(","))
    assert n == len(sigs[name]), (name, n, len(sigs[name]))
    assert hasattr(lib, name)
  assert not set(sigs) & {name for name, _, _ in _lib.SIGNATURES}
  assert lib.rip_head_abi_version() == _lib.HEAD_ABI_VERSION == int(re.search(r"#define RIP_HEAD_ABI_VERSION (\d+)", header).group(1))
  assert lib.rip_abi_version() == _lib.ABI_VERSION


def test_head_is_the_tail_of_the_packed_layout():
  lib = _lib.load()
  spec = arch.packed_spec()
  assert len(R.HEAD_KEYS) == 14 and [k for k, _ in spec[-14:]] == R.HEAD_KEYS and R.HEAD_KEYS[0] == "_merger._model.0.weight"
  assert all(k.startswith("_encoder.") for k, _ in spec[:-14])
  assert lib.rip_head_numel() == R.HEAD_NUMEL == 32164
  assert R.HEAD_NUMEL == sum(int(np.prod(s)) for k, s in spec if not k.startswith("_encoder."))
  packed = W.pack_state_dict(W.synthetic_state_dict(3))
  assert packed.size == arch.packed_numel() and np.array_equal(R.pack_head(W.synthetic_state_dict(3)), packed[-R.HEAD_NUMEL:])
  per_row = 4 * 584 + 456
  assert lib.rip_head_workspace_bytes(4, 512) == 4 * 512 * per_row * 4
  assert lib.rip_head_workspace_bytes(0, 512) == 0 and lib.rip_head_workspace_bytes(9, 1) == 0 and lib.rip_head_workspace_bytes(1, 0) == 0


def _call(**kw):
  """rip_head_forward_backward with fake non-NULL pointers (never dereferenced: every case is refused before a launch)."""
  p = ctypes.c_void_p(0x1000)
  a = dict(head=p, grads=None, feat=p, vec=p, n=8, rows=None, y=p, future=None, L=0, stride=0, noise=None, K=2, B=8,
           max_batch=8, workspace=None, q_rows=p, loss=p, z=None)
  a.update(kw)
  lib = _lib.load()
  rc = lib.rip_head_forward_backward(a["head"], a["grads"], a["feat"], a["vec"], a["n"], a["rows"], a["y"], a["future"], a["L"],
                                     a["stride"], a["noise"], a["K"], a["B"], a["max_batch"], a["workspace"], a["q_rows"],
                                     a["loss"], a["z"], None)
  return rc, lib.rip_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(head=None), "NULL"), (dict(feat=None), "NULL"), (dict(vec=None), "NULL"), (dict(q_rows=None), "NULL"),
    (dict(loss=None), "NULL"), (dict(y=None), "NULL target"), (dict(future=ctypes.c_void_p(0x1000), L=4, stride=1), "exactly one"),
    (dict(noise=ctypes.c_void_p(0x1000)), "noise_dev"),
    (dict(K=0), "K=0"), (dict(K=9), "K=9"), (dict(B=0), "B=0"), (dict(B=9), "B=9 outside [1,max_batch=8]"),
    (dict(n=0, rows=ctypes.c_void_p(0x1000)), "n=0"), (dict(n=7), "n=7 != B=8"),
    (dict(y=None, future=ctypes.c_void_p(0x1000), L=8, stride=1), "stride=1 over L=8"),
    (dict(y=None, future=ctypes.c_void_p(0x1000), L=8, stride=3), "stride=3 over L=8"),
    (dict(y=None, future=ctypes.c_void_p(0x1000), L=3, stride=1), "gives 3 steps"),
    (dict(y=None, future=ctypes.c_void_p(0x1000), L=8, stride=0), "stride=0"),
    (dict(grads=ctypes.c_void_p(0x1000)), "NULL workspace"),
    (dict(head=ctypes.c_void_p(0x1004)), "16-byte aligned"),
])
def test_refusals_before_any_launch(kw, word):
  rc, msg = _call(**kw)
  assert rc == _lib.RIP_EINVAL and word in msg, (rc, msg)


@pytest.mark.parametrize("K, B", sorted(R.CASE_SEEDS))
def test_relu_kink_condition_of_the_gpu_cases(K, B):
  """No pre-activation of the GPU parity cases lies within 1e-4 of a ReLU kink, so a mask decision cannot differ between
  the fp32 kernel and the float64 reference.  Dead units are fine; the (3, 5) case has a merger unit dead on every row."""
  case = R.make_case(K, B)
  assert R.case_min_pre(case) >= R.KINK_MARGIN
  if (K, B) == (3, 5):
    ref = R.head_ref(R.head_model(case["heads"][0]), case["feat"][0], case["vec"], case["y"][0])
    assert np.all(ref["grads"]["_merger._model.0.weight"][R.DEAD_UNIT] == 0.0) and ref["grads"]["_merger._model.0.bias"][R.DEAD_UNIT] == 0.0


@pytest.mark.parametrize("K, B", sorted(R.CASE_SEEDS))
def test_fp32_leaves_room_inside_the_gpu_bound(K, B):
  """The cases are ones fp32 can resolve: torch's own fp32 autograd on them stays within 1e-5 of float64 in the GPU
  tests' metric, a tenth of their bound (head_ref.case_targets says what sets the far-off row's distance)."""
  case = R.make_case(K, B)
  for k in range(K):
    r64 = R.head_ref(R.head_model(case["heads"][k]), case["feat"][k], case["vec"], case["y"][k])
    r32 = R.head_ref(R.head_model(case["heads"][k], torch.float32), case["feat"][k], case["vec"], case["y"][k])
    for key in R.HEAD_KEYS:
      want = r64["grads"][key]
      err = np.abs(r32["grads"][key].astype(np.float64) - want).max() / max(1.0, np.abs(want).max())
      assert err <= 1e-5, (k, key, err)


def test_relu_kink_condition_of_the_real_feature_case():
  """The same for the real-feature case, on the oracle's encoder output for the BEVs the GPU test draws (the kernels'
  features differ from these by about 1e-5, an order below the margin's slack here: 2x the margin is asserted)."""
  case = R.real_case_inputs()
  from oracle import reference_cpu as O
  for k, seed in enumerate(R.MEMBER_SEEDS[:R.REAL_K]):
    m = O.OracleImitativeModel.from_numpy_state_dict(W.synthetic_state_dict(seed))
    with torch.no_grad():
      feat = m._encoder(O.transform_visual(torch.tensor(case["lidar"]).permute(0, 3, 1, 2))).numpy()
    ref = R.head_ref(R.head_model(case["heads"][k]), feat, case["vec"], case["y"][k])
    assert ref["min_pre"] >= 2 * R.KINK_MARGIN, (k, ref["min_pre"])


def test_learning_curve_margin():
  """The learning test's reference curve in float64 and again with the model cast to float32: the largest relative loss
  deviation stays inside `LEARNING_MARGIN` (the figure in this file's docstring), and the float64 curve itself learns."""
  case = R.learning_case()
  c64, c32 = R.learning_curve(case, torch.float64), R.learning_curve(case, torch.float32)
  dev = float(np.max(np.abs(c32 - c64) / np.abs(c64)))
  print("largest relative deviation fp32 vs float64: %.3g; losses %s -> %s" % (dev, c64[0], c64[-1]))
  assert dev <= R.LEARNING_MARGIN
  assert np.all(c64[-1] < c64[0])
