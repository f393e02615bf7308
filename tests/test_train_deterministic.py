"""The deterministic mode of the DIM and CIL training steps (`DIMTrainer(..., deterministic=True)`,
`rip_train_set_option`): with it on, `backward`, `evaluate_step` and `train_epoch` give the same bits
in every trainer and on every run from the same state and inputs; its arithmetic is the default path's up to the order
of the sums; and the steps stay pinned to the reference's recordings (g15, g16).

The batch sizes are the smallest at which each reduction of the step takes its split path (see the case table)."""
import numpy as np
import pytest
import torch

import tests.test_cil_train as cil_tests
import tests.test_gpu_parity as parity
from tests.test_cil_train import make_batch
from tests.test_train_epoch import device_cache, make_trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def dim_case(B, C, dev, seed):
  """(batch, keywords of `backward`) for a DIM step: B synthetic observations as `transform` leaves them, the perturbed
  target and a dropout keep mask."""
  from oatomobile_amd import arch, transform_visual
  rng = np.random.default_rng(seed)
  lidar = ((rng.integers(0, 6, size=(B, 200, 200, C)) / 5.0) * (rng.random((B, 200, 200, C)) < 0.12)).astype(np.float32)
  future = np.cumsum(np.abs(rng.normal(size=(B, arch.T, 2))) * 0.5, axis=1).astype(np.float32)
  batch = dict(visual_features=transform_visual(torch.from_numpy(lidar).to(dev), channels_last=True),
               velocity=torch.from_numpy(rng.normal(0, 3.0, size=(B, 3)).astype(np.float32)).to(dev),
               is_at_traffic_light=torch.from_numpy((rng.random((B, 1)) < 0.2).astype(np.float32)).to(dev),
               traffic_light_state=torch.from_numpy(rng.integers(0, 4, size=(B, 1)).astype(np.float32)).to(dev),
               player_future=torch.from_numpy(future).to(dev))
  y = torch.from_numpy(future + rng.normal(0, 1e-2, size=future.shape).astype(np.float32)).to(dev)
  keep = torch.from_numpy(((rng.random((B, arch.LAST_CHANNELS)) >= 0.2) / 0.8).astype(np.float32)).to(dev)
  return batch, dict(y=y, dropout_mask=keep)


def cil_case(B, T, dev, seed):
  from oatomobile_amd import arch
  rng = np.random.default_rng(seed)
  ctx, _ = make_batch(rng, B, T, dev)
  future = np.cumsum(np.abs(rng.normal(size=(B, T, 2))) * 0.5, axis=1).astype(np.float32)
  keep = torch.from_numpy(((rng.random((B, arch.LAST_CHANNELS)) >= 0.2) / 0.8).astype(np.float32)).to(dev)
  return dict(ctx, player_future=torch.from_numpy(future).to(dev)), dict(dropout_mask=keep)


def trainer(kind, dev, max_batch, C=2, T=4, seed=21, **kw):
  from oatomobile_amd import BehaviouralModel, CILTrainer, DIMTrainer, ImitativeModel
  if kind == "dim":
    return DIMTrainer(ImitativeModel.synthetic(seed, in_channels=C).to(dev), lr=1e-3, max_batch=max_batch, device=dev, **kw)
  return CILTrainer(BehaviouralModel.synthetic(seed, in_channels=C, output_shape=(T, 2)).to(dev), lr=1e-3,
                    max_batch=max_batch, device=dev, **kw)


def output(tr):
  return tr.z if hasattr(tr, "z") else tr.predictions


def step_from(tr, params0, batch, kw):
  """`backward` from the parameters `params0` (a train-mode step updates the running statistics inside `params`):
  clones of the gradient vector, the loss, z / the predictions and the parameters after the step."""
  tr.params.copy_(params0)
  tr.grads.fill_(float("nan"))  # every entry must be written by the step
  loss = tr.backward(batch, **kw)
  return tr.grads.clone(), loss.clone(), output(tr).clone(), tr.params.clone()


def assert_same_bits(a, b, what):
  for name, x, y in zip(("grads", "loss", "z / predictions", "params"), a, b):
    assert torch.isfinite(x).all(), (what, name)
    assert torch.equal(x, y), (what, name, float((x - y).abs().max()))


CASES = [
    # every 50x50 .. 7x7 weight gradient splits (K = 7500 .. 147, ragged against kchunk), the 7x7 stage's forward split
    pytest.param("dim", 2, 3, 4, id="dim-C2-B3"),
    pytest.param("dim", 4, 3, 4, id="dim-C4-B3"),    # the stem's four-channel taps
    pytest.param("dim", 2, 67, 4, id="dim-C2-B67"),  # the 4x4 stage: K = 1072 >= 1024; ragged observation groups in dw_wgrad
    pytest.param("dim", 2, 259, 4, id="dim-C2-B259"),  # the flow-record GEMMs: R = 1036 >= 1024
    pytest.param("cil", 2, 27, 40, id="cil-T40-B27"),  # the decoder-record GEMMs: R = 1080 >= 1024
]


@pytest.mark.parametrize("kind,C,B,T", CASES)
def test_one_step_gives_the_same_bits(dev, kind, C, B, T):
  """Two deterministic trainers built from the same synthetic model, given the same batch, target and dropout mask:
  `torch.equal` on the gradient vector, the loss, z / the predictions and the updated running statistics; and the
  same trainer stepping twice from the restored parameters agrees with itself in the same way."""
  batch, kw = dim_case(B, C, dev, 100 + B) if kind == "dim" else cil_case(B, T, dev, 100 + B)
  a = trainer(kind, dev, B, C=C, T=T, deterministic=True)
  assert a.deterministic
  params0 = a.params.clone()
  first = step_from(a, params0, batch, kw)
  again = step_from(a, params0, batch, kw)
  assert_same_bits(first, again, "one trainer, twice")
  assert float(first[0].abs().max()) > 0
  a.close()
  del a
  b = trainer(kind, dev, B, C=C, T=T, deterministic=True)
  other = step_from(b, params0, batch, kw)
  assert_same_bits(first, other, "two trainers")
  b.close()


@pytest.mark.parametrize("kind,B,T", [("dim", 3, 4), ("cil", 27, 40)])
def test_evaluate_step_gives_the_same_bits(dev, kind, B, T):
  """The forward pass alone (running statistics, no dropout) takes the split-K path too: two `evaluate_step` calls
  give an equal loss and equal z / predictions."""
  batch, _ = dim_case(B, 2, dev, 200 + B) if kind == "dim" else cil_case(B, T, dev, 200 + B)
  tr = trainer(kind, dev, B, T=T, deterministic=True)
  l0 = tr.evaluate_step(batch)
  o0 = output(tr).clone()
  l1 = tr.evaluate_step(batch)
  assert torch.isfinite(l0) and torch.equal(l0, l1) and torch.equal(o0, output(tr))


@pytest.mark.parametrize("kind", ["dim", "cil"])
def test_train_epoch_gives_the_same_bits(tmp_path, dev, kind):
  """Two deterministic trainers run `train_epoch` over 20 datums at batch 8 (steps of 8, 8 and 4 rows) with `clip=True`
  and identically seeded generators: parameters, both Adam moments and the per-batch losses are equal bit for bit.
  (Without the mode two trainers drift apart by up to ~lr per coordinate and step:
  tests/test_train_epoch.py::test_train_epoch_matches_a_replayed_loop.)"""
  _, _, data = device_cache(tmp_path, "train", 20, dev, seed=5)
  done = []
  for _ in range(2):
    _, tr = make_trainer(kind, dev, max_batch=8, deterministic=True)
    loss = tr.train_epoch(data, 8, generator=torch.Generator(device=dev).manual_seed(1234), clip=True)
    done.append((loss, tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.last_epoch_losses.clone()))
    assert tr.step_count == 3
    tr.close()
  (la, *a), (lb, *b) = done
  assert np.isfinite(la) and la == lb
  for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "last_epoch_losses"), a, b):
    assert torch.equal(x, y), (name, float((x - y).abs().max()))


REFERENCE_RUNS = 32  # a decision that flips once in 30 runs is still seen two times in three


def decidable_case(kind, B, T, dev, ref, params0):
  """A batch at which the comparison with the default path can be decided: the first of the seeds 300 + B, 1300 + B, ...
  at which REFERENCE_RUNS default steps from `params0` give gradient vectors within 5e-5 (relative L2) of the first.

  The step is piecewise linear (ReLU6, ReLU, the CIL L1 loss), and the default path's atomics move its forward pass in
  the last place, so an activation that lies within ~1e-7 of a kink is decided one way in one run and the other way in
  the next.  A batch either has such an activation or not.  Measured on the MI355X over 80 default steps from one
  state: DIM B = 3 at seed 303 gives one of two gradients, 1.9e-3 apart, about evenly (consecutive runs differ in 40
  of 79 pairs; every other difference is ~1.5e-6); CIL B = 27 at seed 327 three, up to 3.9e-4 apart (27 of 79), and
  four of the first five CIL batches spread by 1.4e-4 .. 3.8e-3 (B = 27 splits the forward pass from the 7x7 stage on:
  ten million ReLU6 decisions behind it).  At such a batch "the default path's gradient" is not one vector at the 1e-4 the comparison is held to, whatever is compared
  with it; the selection looks at the default path alone, never at the deterministic one.  For CIL the targets are put
  0.6 .. 1.5 from the predictions of a train-mode forward pass, as
  tests/test_cil_train.py::test_cil_backward_vs_restatement_same_kinks does for the L1 kink (margin asserted by the
  caller).  Returns (batch, keywords, the first default step, the spread of the others around it)."""
  for seed in range(300 + B, 300 + B + 20 * 1000, 1000):
    batch, kw = dim_case(B, 2, dev, seed) if kind == "dim" else cil_case(B, T, dev, seed)
    if kind == "cil":
      ref.params.copy_(params0)
      ref.backward(batch, gradients=False, **kw)
      rng = np.random.default_rng(seed)
      off = (rng.choice([-1.0, 1.0], size=(B, T, 2)) * rng.uniform(0.6, 1.5, size=(B, T, 2))).astype(np.float32)
      batch = dict(batch, player_future=ref.predictions + torch.from_numpy(off).to(dev))
    first = step_from(ref, params0, batch, kw)
    norm = torch.linalg.vector_norm(first[0].double())
    spread = max(float(torch.linalg.vector_norm((step_from(ref, params0, batch, kw)[0] - first[0]).double()) / norm)
                 for _ in range(REFERENCE_RUNS - 1))
    print("%s B=%d seed %d: %d default steps within %.3g of the first" % (kind, B, seed, REFERENCE_RUNS, spread))
    if spread <= 5e-5:
      return batch, kw, first, spread
  pytest.fail("the default path does not reproduce itself to 5e-5 at any of 20 batches")


@pytest.mark.parametrize("kind,B,T", [("dim", 3, 4), ("dim", 67, 4), ("cil", 27, 40)])
def test_same_arithmetic_as_the_default_path(dev, kind, B, T):
  """From the same state and inputs the mode computes what the default path computes, up to the order of the sums: the
  loss within 1e-6 relative (the run-to-run tolerance two default forward passes are held to) and the whole packed
  gradient vector within 1e-4 in relative L2 (the project's fp32 parity contract).  Gradients, not post-Adam
  parameters: a zero-gradient parameter moves by +-lr with a noise-determined sign.  The batch is one at which the
  default path reproduces its own gradient to half that bound (`decidable_case`).

  Measured on the MI355X (`pytest -s`): relative L2 against the default path 1.5e-6 (DIM B = 3), 3.5e-7 and 2.7e-5 in
  different processes (DIM B = 67; two default runs of the same process differ by the same figure), 8.6e-6 (CIL
  B = 27, T = 40; two default runs 1.2e-5); loss differences at most 2.7e-7."""
  det = trainer(kind, dev, B, T=T, deterministic=True)
  ref = trainer(kind, dev, B, T=T)
  assert not ref.deterministic
  params0 = ref.params.clone()
  batch, kw, (gr, lr_, orf, _), own = decidable_case(kind, B, T, dev, ref, params0)
  gd, ld, od, _ = step_from(det, params0, batch, kw)
  if kind == "cil":
    margin = min(float((o - batch["player_future"]).abs().min()) for o in (od, orf))
    assert margin > 0.5, margin
  rel_loss = abs(float(ld) - float(lr_)) / abs(float(lr_))
  rel_l2 = float(torch.linalg.vector_norm((gd - gr).double()) / torch.linalg.vector_norm(gr.double()))
  print("%s B=%d: loss %.7g (default %.7g, relative %.2g), gradient relative L2 %.3g (default runs among themselves: "
        "%.3g), max|d output| %.2g" % (kind, B, float(ld), float(lr_), rel_loss, rel_l2, own, float((od - orf).abs().max())))
  assert rel_loss <= 1e-6
  assert rel_l2 <= 1e-4


def test_g15_dim_step_pinned_to_the_reference(golden, dev, monkeypatch):
  """The g15 recording of the reference's two DIM training steps, through the existing test's checks and tolerances
  (tests/test_gpu_parity.py::test_g15_train_step_vs_reference) with the trainer it builds switched to the mode."""
  import oatomobile_amd
  built = []

  class Deterministic(oatomobile_amd.DIMTrainer):

    def __init__(self, *args, **kw):
      super().__init__(*args, deterministic=True, **kw)
      built.append(self)

  monkeypatch.setattr(oatomobile_amd, "DIMTrainer", Deterministic)
  parity.test_g15_train_step_vs_reference(golden, dev)
  assert len(built) == 1 and built[0].deterministic and built[0].step_count == 2


def test_g16_cil_step_pinned_to_the_reference(golden, dev, monkeypatch):
  """The g16 recording of the reference's two CIL training steps, through
  tests/test_cil_train.py::test_g16_cil_train_step_vs_reference with its trainer switched to the mode."""
  import oatomobile_amd
  built = []

  class Deterministic(oatomobile_amd.CILTrainer):

    def __init__(self, *args, **kw):
      super().__init__(*args, deterministic=True, **kw)
      built.append(self)

  monkeypatch.setattr(oatomobile_amd, "CILTrainer", Deterministic)
  cil_tests.test_g16_cil_train_step_vs_reference(golden, dev)
  assert len(built) == 1 and built[0].deterministic and built[0].step_count == 2


@pytest.mark.parametrize("kind", ["dim", "cil"])
def test_switch(dev, kind):
  """`rip_train_set_option` on DIM and CIL handles: an unknown option or value is RIP_EINVAL and changes nothing; on,
  off, on again works, and the result after off-then-on equals the result before, bit for bit; a trainer is built
  with the mode off."""
  from oatomobile_amd import _lib
  lib = _lib.load()
  B, T = 3, 4
  batch, kw = dim_case(B, 2, dev, 400) if kind == "dim" else cil_case(B, T, dev, 400)
  tr = trainer(kind, dev, B, T=T)
  assert tr.deterministic is False
  with pytest.raises(AttributeError):
    tr.deterministic = True  # read-only
  assert lib.rip_train_set_option(tr._h, 99, 1) == _lib.RIP_EINVAL
  assert lib.rip_train_set_option(tr._h, _lib.TRAIN_OPT_DETERMINISTIC, 2) == _lib.RIP_EINVAL
  assert lib.rip_train_set_option(tr._h, _lib.TRAIN_OPT_DETERMINISTIC, -1) == _lib.RIP_EINVAL
  assert lib.rip_train_set_option(None, _lib.TRAIN_OPT_DETERMINISTIC, 1) == _lib.RIP_EINVAL
  params0 = tr.params.clone()
  _lib.check(lib.rip_train_set_option(tr._h, _lib.TRAIN_OPT_DETERMINISTIC, 1))
  _lib.check(lib.rip_train_set_option(tr._h, _lib.TRAIN_OPT_DETERMINISTIC, 1))  # on twice: the workspace is kept
  before = step_from(tr, params0, batch, kw)
  _lib.check(lib.rip_train_set_option(tr._h, _lib.TRAIN_OPT_DETERMINISTIC, 0))
  off = step_from(tr, params0, batch, kw)  # the default path again: equal to rounding
  assert float((off[0] - before[0]).norm() / before[0].norm()) <= 1e-4
  _lib.check(lib.rip_train_set_option(tr._h, _lib.TRAIN_OPT_DETERMINISTIC, 0))  # off twice
  _lib.check(lib.rip_train_set_option(tr._h, _lib.TRAIN_OPT_DETERMINISTIC, 1))
  after = step_from(tr, params0, batch, kw)
  assert_same_bits(before, after, "off, then on again")
  tr.close()
