"""Training by the epoch from a device-resident cache: `replay.DeviceCache` (`rip_gather_batch_u8`, the batch assembly
kernel), `DIMTrainer` / `CILTrainer.train_epoch` and `evaluate_epoch` (dim/train.py:215-266, cil/train.py:192-236),
the data-parallel epoch and the command-line training of `oatomobile_amd.baselines.torch.{dim,cil}.train`."""
import ctypes
import glob
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import synth_observation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODALITIES = ("lidar", "is_at_traffic_light", "traffic_light_state", "player_future", "velocity")


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def write_datums(split_dir, n, C=2, L=80, seed=0):
  """`n` synthetic datum files in `split_dir` (replay.Episode: <parent>/<token>/*.npz); futures of every driving mode,
  the motion loosely tied to the velocity so that there is something to learn.  Returns the sorted file list (the
  order of `replay.as_torch`)."""
  from oatomobile_amd import replay
  ep = replay.Episode(os.path.dirname(split_dir), os.path.basename(split_dir))
  rng = np.random.default_rng(seed)
  for i in range(n):
    o = synth_observation(np.random.default_rng(seed * 1000 + i), C=C)
    heading = rng.choice([0.0, 0.5, -0.5])
    speed = 0.02 if i % 7 == 0 else 0.3 + 0.1 * abs(float(o["velocity"][0]))
    steps = speed * (1.0 + 0.1 * rng.normal(size=(L, 1)))
    fut = np.concatenate([np.cumsum(steps * np.cos(heading), 0), np.cumsum(steps * np.sin(heading), 0),
                          rng.normal(size=(L, 1))], axis=1).astype(np.float32)
    ep.append("d%04d" % i, lidar=o["lidar"], velocity=o["velocity"], is_at_traffic_light=o["is_at_traffic_light"],
              traffic_light_state=o["traffic_light_state"], player_future=fut)
  return sorted(glob.glob(os.path.join(split_dir, "*.npz")))


def device_cache(tmp_path, name, n, dev, C=2, seed=0):
  from oatomobile_amd import replay
  files = write_datums(str(tmp_path / name), n, C=C, seed=seed)
  cache = replay.pack_cache(files, str(tmp_path / (name + "_cache")), workers=1, targets=True)
  return files, cache, replay.DeviceCache(cache, dev)


def reference_batch(files, rows, model, dev):
  """The reference's data path for `rows`: `as_torch(mode=True)` items -> default collate -> `.to(device)` ->
  `model.transform` (dim/train.py:122-134)."""
  from oatomobile_amd import replay
  ds = replay.as_torch(os.path.dirname(files[0]), modalities=MODALITIES, mode=True)
  batch = torch.utils.data.default_collate([ds[int(i)] for i in rows])
  return model.transform({k: v.to(dev) for k, v in batch.items()})


# ---------------------------------------------------------------------------------------------------------
# the assembly kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_gather_batch_is_exact(tmp_path, dev, C):
  """`DeviceCache.batch` == `transform_visual(lut[codes[rows]], channels_last=True)` bit for bit (C = 4: per channel
  pair, see below), and the vec /
  target / mode gathers == their numpy gathers (random rows with repeats, B = 37, T = 4 and T = 40)."""
  from oatomobile_amd import transform_visual
  files, cache, data = device_cache(tmp_path, "g", 29, dev, C=C, seed=3 + C)
  rng = np.random.default_rng(C)
  rows = rng.integers(0, 29, size=37)
  rows[5] = rows[20]  # a repeat for sure
  for T in (4, 40):
    stride = 80 // T
    batch = data.batch(torch.from_numpy(rows).to(dev), T, mode=True)
    lidar = torch.from_numpy(cache.lut[np.asarray(cache.codes)[rows]]).to(dev)
    want = transform_visual(lidar, channels_last=True)
    assert batch["visual_features"].shape == (37, C, 100, 100)
    if C <= 3:
      np.testing.assert_array_equal(batch["visual_features"].cpu().numpy(), want.cpu().numpy())
    else:
      # rip_transform takes its untiled kernel at C = 4: same formula, the compiler contracts it differently, so the
      # two differ by one rounding on ~0.1 % of the elements.  The interpolation is per channel: channel pairs through
      # the tiled C = 2 transform are the exact reference.
      pairs = torch.cat([transform_visual(lidar[..., c:c + 2].contiguous(), channels_last=True) for c in (0, 2)], dim=1)
      np.testing.assert_array_equal(batch["visual_features"].cpu().numpy(), pairs.cpu().numpy())
      np.testing.assert_allclose(batch["visual_features"].cpu().numpy(), want.cpu().numpy(), rtol=0, atol=2.4e-7)
    np.testing.assert_array_equal(batch["velocity"].cpu().numpy(), cache.vec[rows, 0:3])
    np.testing.assert_array_equal(batch["is_at_traffic_light"].cpu().numpy(), cache.vec[rows, 3:4])
    np.testing.assert_array_equal(batch["traffic_light_state"].cpu().numpy(), cache.vec[rows, 4:5])
    np.testing.assert_array_equal(batch["player_future"].cpu().numpy(), np.asarray(cache.future)[rows, 0::stride])
    mode = np.asarray(cache.mode)[rows].copy()
    mode[mode == 1.0] = 0.0  # cil/model.py:166-168
    np.testing.assert_array_equal(batch["mode"].cpu().numpy(), mode[:, None])
  # host rows: range-checked before any launch; a slice that does not give T steps is refused
  np.testing.assert_array_equal(data.batch(rows.tolist(), 4)["visual_features"].cpu().numpy(),
                                data.batch(torch.from_numpy(rows).to(dev), 4)["visual_features"].cpu().numpy())
  with pytest.raises(IndexError):
    data.batch([0, 29], 4)
  with pytest.raises(ValueError):
    data.batch(rows, 3)



@pytest.mark.gpu
def test_gather_batch_row_outside_the_cache_gives_nan(tmp_path, dev):
  """A device row outside [0, n) is not range-checked on the host (that would synchronise): the kernel reads nothing
  for it and writes NaN into that row's outputs; the other rows of the batch are unaffected."""
  _, _, data = device_cache(tmp_path, "g", 7, dev, seed=9)
  rows = torch.tensor([3, 7, 0, -1, 6], device=dev, dtype=torch.int64)
  batch = data.batch(rows, 4, mode=True)
  good = data.batch(torch.tensor([3, 0, 6], device=dev, dtype=torch.int64), 4, mode=True)
  for key in ("visual_features", "velocity", "is_at_traffic_light", "traffic_light_state", "player_future", "mode"):
    v = batch[key]
    assert torch.isnan(v[[1, 3]]).all(), key
    assert torch.equal(v[[0, 2, 4]], good[key]), key


@pytest.mark.gpu
def test_gather_batch_row_offsets_above_2_31_bytes(dev):
  """A code tensor of 28 000 rows of 200 x 200 x 2 (2.24 GB) made on the device; rows near its end sit beyond 2^31
  bytes, so a 32-bit row offset would read the wrong rows.  `rip_gather_batch_u8` through ctypes."""
  from oatomobile_amd import _lib, transform_visual
  n, H, W, C, L, T = 28000, 200, 200, 2, 80, 4
  if torch.cuda.mem_get_info(dev)[0] < 4 * n * H * W * C:
    pytest.fail("needs %.1f GB of free device memory" % (4 * n * H * W * C / 1e9))
  codes = torch.zeros((n, H, W, C), dtype=torch.uint8, device=dev)
  g = torch.Generator(device=dev).manual_seed(5)
  tail = torch.randint(0, 6, (8, H, W, C), device=dev, generator=g, dtype=torch.int64).to(torch.uint8)
  codes[n - 8:] = tail
  lut = torch.full((256,), float("nan"), device=dev)
  lut[:6] = torch.arange(6, device=dev, dtype=torch.float32) / 5.0
  vec = torch.arange(n * 5, device=dev, dtype=torch.float32).reshape(n, 5)
  future = torch.arange(n * L * 2, device=dev, dtype=torch.float32).reshape(n, L, 2)
  mode = torch.arange(n, device=dev, dtype=torch.float32) % 4
  rows = torch.tensor([n - 1, n - 8, n - 3, 0, n - 1, n - 5], device=dev, dtype=torch.int64)
  assert int(rows[0]) * H * W * C > 2**31
  B = rows.numel()
  visual = torch.empty((B, C, 100, 100), device=dev)
  vec_out = torch.empty((B, 5), device=dev)
  target = torch.empty((B, T, 2), device=dev)
  mode_out = torch.empty((B, 1), device=dev)
  lib = _lib.load()
  _lib.check(lib.rip_gather_batch_u8(_lib.ptr(codes, torch.uint8), _lib.ptr(lut), _lib.ptr(rows, torch.int64), B, n, C, H, W,
                                     100, _lib.ptr(vec), _lib.ptr(future), L, T, L // T, _lib.ptr(mode), _lib.ptr(visual),
                                     _lib.ptr(vec_out), _lib.ptr(target), _lib.ptr(mode_out), _lib.current_stream(dev)))
  want = transform_visual(lut[codes[rows].long()], channels_last=True)
  assert torch.equal(visual, want)
  assert float(visual[0].abs().sum()) > 0  # the random tail, not the zeros in front of it
  assert torch.equal(vec_out, vec[rows])
  assert torch.equal(target, future[rows, 0::L // T])
  want_mode = mode[rows].clone()
  want_mode[want_mode == 1.0] = 0.0
  assert torch.equal(mode_out[:, 0], want_mode)
  del codes
  torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------
# evaluate_epoch / train_epoch against hand-written loops over the reference's data path
# ---------------------------------------------------------------------------------------------------------
def make_trainer(kind, dev, max_batch, T=4, seed=21, **kw):
  from oatomobile_amd import BehaviouralModel, CILTrainer, DIMTrainer, ImitativeModel
  if kind == "dim":
    model = ImitativeModel.synthetic(seed).to(dev)
    return model, DIMTrainer(model, lr=1e-3, max_batch=max_batch, device=dev, **kw)
  model = BehaviouralModel.synthetic(seed, output_shape=(T, 2)).to(dev)
  return model, CILTrainer(model, lr=1e-3, max_batch=max_batch, device=dev, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dim", "cil"])
def test_evaluate_epoch_matches_evaluate_step_loop(tmp_path, dev, kind):
  """`evaluate_epoch(data, bs)` == mean over the same partition of `evaluate_step` on batches built the existing way
  (`as_torch` -> `.to(dev)` -> `model.transform`), at 1e-6 relative.  bs = 10 > max_batch = 4: the 5x validation
  batch, evaluated in chunks and recombined as the row-weighted mean of the chunk means."""
  files, _, data = device_cache(tmp_path, "val", 23, dev, seed=11)
  model, trainer = make_trainer(kind, dev, max_batch=4)
  _, wide = make_trainer(kind, dev, max_batch=16)  # the same weights: evaluates a whole batch in one step
  for bs in (4, 10):
    got = trainer.evaluate_epoch(data, bs)
    want = [float(wide.evaluate_step(reference_batch(files, range(i, min(i + bs, 23)), model, dev)))
            for i in range(0, 23, bs)]
    assert trainer.last_epoch_losses.shape == (len(want),)
    np.testing.assert_allclose(trainer.last_epoch_losses.cpu().numpy(), want, rtol=1e-6)
    assert abs(got - float(np.mean(want))) <= 1e-6 * abs(np.mean(want)), (got, np.mean(want))
  # shuffled: the order of torch.randperm(n, generator=g), kept in last_permutation
  g = torch.Generator(device=dev).manual_seed(8)
  got = trainer.evaluate_epoch(data, 10, generator=g, shuffle=True)
  perm = trainer.last_permutation.cpu().numpy()
  assert np.array_equal(perm, torch.randperm(23, device=dev, generator=torch.Generator(device=dev).manual_seed(8)).cpu().numpy())
  want = [float(wide.evaluate_step(reference_batch(files, perm[i:i + 10], model, dev))) for i in range(0, 23, 10)]
  assert abs(got - float(np.mean(want))) <= 1e-6 * abs(np.mean(want)), (got, np.mean(want))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dim", "cil"])
def test_train_epoch_matches_a_replayed_loop(tmp_path, dev, kind):
  """`train_epoch` with a seeded generator == a hand-written loop that replays its draws in the documented order
  (permutation; per batch the DIM target noise, then the dropout keep mask) on batches built the existing way.

  Every replayed step starts from the state the epoch had before that step (parameters with the BatchNorm running
  statistics, Adam moments, step and batch counters, captured around `backward`).  The training kernels reduce
  weight gradients with unordered float atomics, so two trainers running freely drift apart by up to ~lr per
  coordinate per Adam step; from an identical state, a step's inputs are equal bit for bit (visual features, target
  noise, dropout mask) and its loss is a forward pass, held at the forward pass's run-to-run tolerance (1e-6, as
  tests/test_cil_train.py holds two evaluate_step calls)."""
  from oatomobile_amd import arch
  files, _, data = device_cache(tmp_path, "train", 20, dev, seed=5)
  _, a = make_trainer(kind, dev, max_batch=8)
  model, b = make_trainer(kind, dev, max_batch=8)
  states = []
  backward = a.backward

  def capturing_backward(batch, **kw):
    states.append(dict(params=a.params.clone(), exp_avg=a.exp_avg.clone(), exp_avg_sq=a.exp_avg_sq.clone(),
                       step_count=a.step_count, num_batches_tracked=a.num_batches_tracked,
                       visual=batch["visual_features"].clone(), y=None if kw.get("y") is None else kw["y"].clone(),
                       keep=kw["dropout_mask"].clone()))
    return backward(batch, **kw)

  a.backward = capturing_backward
  ga = torch.Generator(device=dev).manual_seed(1234)
  loss = a.train_epoch(data, 8, generator=ga, clip=True)  # batches of 8, 8 and 4 rows (drop_last=False)
  got = a.last_epoch_losses.cpu().numpy()
  assert got.shape == (3,) and len(states) == 3
  assert abs(loss - float(np.mean(got))) <= 1e-6 * abs(loss)
  gb = torch.Generator(device=dev).manual_seed(1234)
  perm = torch.randperm(20, device=dev, generator=gb)
  assert torch.equal(perm, a.last_permutation)
  for k, i in enumerate(range(0, 20, 8)):
    st = states[k]
    b.params.copy_(st["params"])
    b.exp_avg.copy_(st["exp_avg"])
    b.exp_avg_sq.copy_(st["exp_avg_sq"])
    b.step_count, b.num_batches_tracked = st["step_count"], st["num_batches_tracked"]
    batch = reference_batch(files, perm[i:i + 8].cpu().numpy(), model, dev)
    B = batch["visual_features"].shape[0]
    assert torch.equal(batch["visual_features"], st["visual"])
    kw = {}
    if kind == "dim":
      target = batch["player_future"][..., :2]
      kw["y"] = target + torch.empty(target.shape, device=dev).normal_(0.0, 1e-2, generator=gb)
      assert torch.equal(kw["y"], st["y"])
    else:
      assert st["y"] is None
    keep = torch.empty(B, arch.LAST_CHANNELS, device=dev).bernoulli_(0.8, generator=gb).mul_(1.0 / 0.8)
    assert torch.equal(keep, st["keep"])
    want = float(b.train_step(batch, dropout_mask=keep, clip=True, **kw))
    assert abs(got[k] - want) <= 1e-6 * abs(want), (k, got[k], want)
  assert a.step_count == b.step_count == 3 and a.num_batches_tracked == b.num_batches_tracked
  # the last step from the same state: Adam moves a coordinate by at most lr (1 - beta1) / sqrt(1 - beta2) ~ 3.2 lr,
  # so two roundings of a tiny gradient of opposite sign put two runs at most ~6.4 lr apart; most agree far closer
  tr = a._trainable.bool()
  d = (a.params - b.params)[tr]
  assert float(d.abs().max()) <= 6.4e-3, float(d.abs().max())
  assert float(d.norm() / b.params[tr].norm()) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dim", "cil"])
def test_epochs_lower_train_and_val_loss(tmp_path, dev, kind):
  """Several epochs on a small synthetic set lower both the training loss (last epochs against the first) and the
  validation loss (last epochs against the untrained model's)."""
  _, _, train = device_cache(tmp_path, "train", 48, dev, seed=1)
  _, _, val = device_cache(tmp_path, "val", 16, dev, seed=2)
  _, trainer = make_trainer(kind, dev, max_batch=16)
  g = torch.Generator(device=dev).manual_seed(0)
  val0 = trainer.evaluate_epoch(val, 80)
  tl, vl = [], []
  for _ in range(8):
    tl.append(trainer.train_epoch(train, 16, generator=g))
    vl.append(trainer.evaluate_epoch(val, 80))
  assert all(np.isfinite(tl + vl))
  assert np.mean(tl[-2:]) < tl[0], tl
  # the validation loss is noisy epoch to epoch (16 observations, lr 1e-3): compared with the untrained model
  assert np.mean(vl[-3:]) < val0 and min(vl) < val0, (val0, vl)


# ---------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dim", "cil"])
def test_command_line_training(tmp_path, kind):
  """`python -m oatomobile_amd.baselines.torch.<kind>.train` for 2 epochs at batch 8: checkpoints every epoch
  (--save_model_frequency 1) that load strict=True into this package's model and into the oracle's restatement of
  the reference class; metrics.jsonl has one line per epoch and split; a second run reuses the packed cache."""
  from oatomobile_amd import BehaviouralModel, ImitativeModel
  from oracle.cil import OracleBehaviouralModel
  from oracle.reference_cpu import OracleImitativeModel
  ds = tmp_path / "dataset"
  write_datums(str(ds / "train"), 12, seed=1)
  write_datums(str(ds / "val"), 5, seed=2)
  out = tmp_path / "out"
  cmd = [sys.executable, "-m", "oatomobile_amd.baselines.torch.%s.train" % kind, "--dataset_dir", str(ds), "--output_dir",
         str(out), "--num_epochs", "2", "--batch_size", "8", "--save_model_frequency", "1", "--clip_gradients"]
  r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-3000:]
  assert sorted(os.listdir(out / "ckpts")) == ["model-0.pt", "model-1.pt"]
  for name in ("model-0.pt", "model-1.pt"):
    sd = torch.load(out / "ckpts" / name, map_location="cpu")
    if kind == "dim":
      ImitativeModel().load_state_dict(sd, strict=True)
      OracleImitativeModel().load_state_dict(sd, strict=True)
    else:
      BehaviouralModel(output_shape=(4, 2)).load_state_dict(sd, strict=True)
      OracleBehaviouralModel(output_shape=(4, 2)).load_state_dict(sd, strict=True)
    assert all(torch.isfinite(v.float()).all() for v in sd.values())
  lines = [json.loads(l) for l in open(out / "logs" / "metrics.jsonl")]
  assert [(l["epoch"], l["split"]) for l in lines] == [(0, "train"), (0, "val"), (1, "train"), (1, "val")]
  for l in lines:
    assert np.isfinite(l["loss"]) and l["observations_per_s"] > 0
    assert l["observations"] == (12 if l["split"] == "train" else 5)
    assert ("nll_limit" in l) == (kind == "dim")
  if kind == "dim":
    assert abs(lines[0]["nll_limit"] - (4 * np.log(2 * np.pi) + 8 * np.log(1e-2))) < 1e-4
  assert sorted(os.listdir(out / "cache")) == ["train", "val"]
  stamp = os.path.getmtime(out / "cache" / "train" / "codes.npy")
  cmd[cmd.index("--num_epochs") + 1] = "1"
  r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-3000:]
  assert os.path.getmtime(out / "cache" / "train" / "codes.npy") == stamp  # reused, not repacked


# ---------------------------------------------------------------------------------------------------------
# data parallel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_train_epoch_two_ranks(tmp_path):
  """`train_epoch` under `group=` as two gloo processes sharing one GPU (tests/mp/train_epoch_two_ranks.py): both
  ranks draw the same permutation, their rows per global batch are disjoint and cover it (the last global batch has
  one row: rank 1 joins the all-reduce with an empty slice), the trainable parameters are identical after the
  epoch, and both ranks return the same row-weighted losses."""
  from oatomobile_amd import replay
  files = write_datums(str(tmp_path / "train"), 13, seed=4)
  replay.pack_cache(files, str(tmp_path / "cache"), workers=1, targets=True)
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
  env = dict(os.environ, RIP_BENCH_SHARE_GPU="1", RIP_BENCH_BACKEND="gloo")
  for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
    env.pop(k, None)
  out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "mp", "train_epoch_two_ranks.py"),
                        str(tmp_path / "cache")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
  assert out.returncode == 0, out.stderr[-3000:]
  rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
  assert rec["world"] == 2 and rec["same_permutation"], rec
  assert rec["global_batches"] == 3 and rec["rows_per_rank"] == [[3, 3, 1], [3, 3, 0]], rec
  assert rec["disjoint_and_cover"], rec
  assert rec["params_identical"] and np.isfinite(rec["loss"]), rec
  assert rec["losses_identical"] and len(rec["batch_losses"]) == 3, rec
